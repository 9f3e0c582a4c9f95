"""Autograd glue of the HIP training path.

``LFIntegrator.forward`` (enflow/flow/dynamics.py:10-24) and
``Alchemical_NLL.__call__`` (enflow/flow/loss.py:21-24) become
``torch.autograd.Function`` s whose backward passes call the C ABI
(enflow_alchemical_nll_backward_f32, enflow_lf_backward_f32).  Parameters
enter the flow function as inputs, so ``loss.backward()`` fills every
``p.grad`` exactly like the reference's autograd, and DDP / optimisers / LR
schedulers work on them unchanged (enflow/main.py:212-223).
"""
import ctypes
import math
import os

import torch
from torch.autograd.function import once_differentiable

from .. import _lib
from ..nn._act import check_trainable
from ..nn.argmax import ArgMax
from ..nn._pad import ARGMAX_HDIMS, EGCL_HDIMS, unpad_grads
from .dynamics import _fp32_prec, _host_noise, _retry_fp32


def pair_row_bound(N):
    """Upper bound of the backward's pair rows: sum of n(n-1) rounded up to 32."""
    N = torch.as_tensor(N).reshape(-1).to(torch.int64)
    return int((((N * (N - 1)) + 31) // 32 * 32).sum())


def _adj(t, shape, dev, clone=False):
    """An incoming gradient as a contiguous fp32 adjoint of `shape` (zeros for
    None); clone: a private copy the kernels update in place."""
    if t is None:
        return torch.zeros(shape, dtype=torch.float32, device=dev)
    t = t.detach().to(dtype=torch.float32)
    return t.contiguous().clone() if clone else t.reshape(shape).contiguous()


def _alloc_ws(nbytes, what, dev):
    """The uint8 workspace of a C entry from its *_workspace_size answer
    (negative: the entry's own refusal, `what`)."""
    if nbytes < 0:
        raise _lib.HipPathError(what)
    return torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)


_warned_bf16 = []


def _tape_prec(flow):
    """The flow's GEMM precision for a taped pass: the tape feeds the
    fp32-accurate backward, so bf16 records at f16x3 (warned once)."""
    prec = flow._prec()
    if (prec & 0xff) == _lib.PREC_BF16:
        prec = (prec & ~0xff) | _lib.PREC_F16X3
        if not _warned_bf16:
            _warned_bf16.append(True)
            import warnings
            warnings.warn("enflow_amd: gemm_precision='bf16' is a generate-path setting; the training "
                          "forward runs f16x3", RuntimeWarning, stacklevel=3)
    return prec


def _bwd_section(net, dev):
    """One standalone EGCL's (raw, bwd): its flat parameters at the kernel width
    (att_nn.0's slots zero without attention) and the backward's packed section."""
    L = _lib.lib(net.kernel_nf)
    hid, nf = net.kernel_hidden, net.kernel_nf
    raw = torch.cat([net.kernel_raw(dev), net._att_raw(dev) if net.attention else torch.zeros(hid + 1, device=dev)])
    bwd = torch.empty(max(L.enflow_egcl_bwd_packed_size(hid, nf), 1), dtype=torch.float32, device=dev)
    _lib.check(L.enflow_pack_egcl_bwd_f32(_lib.ptr(raw), hid, nf, _lib.ptr(bwd), _lib.stream_ptr(dev)),
               "enflow_pack_egcl_bwd_f32")
    return raw, bwd


def _padded_g_adjoint(gg, n, nf, net, dev):
    """d G at the kernel width: G's padded columns get no adjoint."""
    ag = torch.zeros((n, nf), dtype=torch.float32, device=dev)
    if gg is not None:
        ag[:, :net.output_nf] = gg.detach().to(torch.float32).reshape(n, net.output_nf)
    return ag


def _apply_to_data(fn, flow, meta, data, dev, dequantize=False):
    """fn.apply on the data's fp32 state on `dev` and the flow's parameters (the
    layers', then an ArgMax dequantiser's if it takes part); the five outputs."""
    params = [p for n in flow.networks for _, p in n.named_parameters()]
    if dequantize and isinstance(flow.dequantize, ArgMax):
        params += list(flow.dequantize.parameters())
    return fn.apply(flow, meta, *(t.to(device=dev, dtype=torch.float32)
                                  for t in (data.h, data.g, data.pos, data.vel)), *params)


def _write_back(data, h, g, pos, vel, ldj):
    """The outputs into `data` at its own dtypes; returns (data, ldj)."""
    dt = data.h.dtype
    data.h, data.g = h.to(dt), g.to(dt)
    data.pos, data.vel = pos.to(data.pos.dtype), vel.to(data.vel.dtype)
    return data, ldj.to(dt)


class _FlowFunction(torch.autograd.Function):
    """LFIntegrator.forward with the HIP backward.  meta["per_molecule"]
    (LFIntegrator.forward_grad): the fifth output is the [num_mols] log|detJ| the
    forward launch writes per molecule (with ArgMax plus each molecule's share of
    the batch constant, as forward(per_molecule=True)) instead of their total, and
    the backward takes a [num_mols] upstream gradient for it: expanded to one value
    per atom (enflow_ldj_mol_to_atoms_f32) and read by the same backward entries
    under ENFLOW_BWD_LDJ_ATOMS."""

    @staticmethod
    def forward(ctx, flow, meta, h, g, pos, vel, *params):
        hid, nf, cw = flow._geometry()
        kind = flow._dequant_kind()
        dev = h.device
        L = _lib.lib(nf)
        n_layers = len(flow.networks)
        A = h.shape[0]
        M = meta["mol_ptr"].numel() - 1
        # out of place: the kernel reads the inputs and writes fresh outputs (the
        # input h is kept for the dequantiser's backward as is, no copy)
        src = tuple(t.detach().contiguous() for t in (h, g, pos, vel))
        h_in = src[0]
        hw, gw, pw, vw = (torch.empty_like(t) for t in src)
        tape = torch.empty(max(L.enflow_lf_tape_size_for(A, nf, hid, n_layers, meta["max_n"]), 1),
                           dtype=torch.float32, device=dev)
        # fused: unique pairs [n_layers][M]; large: the backward's pair rows per layer
        counts = torch.zeros(max(n_layers * (1 if meta["large"] else M), 1), dtype=torch.int32, device=dev)
        ldj_mol = torch.empty(max(M, 1), dtype=torch.float32, device=dev)
        ldj = torch.empty(1, dtype=torch.float32, device=dev)
        st = torch.zeros(2, dtype=torch.int32, device=dev)   # error word, ldj reduction ticket
        err = st[:1]
        prec = _tape_prec(flow)
        # both packed sections of every layer first (training_layers: after an
        # optimiser step, two launches per section for the whole flow, ABI 13), so
        # the forward launch reuses the forward section (packed_layers' cache); the
        # buffers and the parameter versions they were packed from go with this
        # graph: the backward uses exactly these and refuses in-place changes since
        ctx.train_bufs = flow.training_layers(dev)
        ctx.train_key = flow._params_key(dev)
        flow.forward_buffers(hw, gw, pw, vw, meta["box"], meta["r_cut"], meta["mol_ptr"], meta["max_n"],
                             meta["noise"], ldj_mol, ldj, err, tape=tape, pair_counts=counts, prec=prec,
                             src=src, ticket=st[1:])
        # an fp32-GEMM forward's tape gets the fp32-GEMM backward (ENFLOW_BWD_F32)
        ctx.bwd_f32 = (prec & 0xff) == _lib.PREC_F32
        # the dequantiser's flat parameters behind the forward kernel, ahead of the
        # error check's sync
        ctx.dq_raw = None
        if kind == _lib.DEQUANT_ARGMAX:
            ctx.dq_raw = flow.dequantize.kernel_raw(dev, hid)
        if meta["check_errors"]:
            if getattr(flow, "defer_error_check", False):
                # no host sync: the word is read at the start of this graph's
                # backward (before anything consumes the outputs' gradients) or
                # at the next check; an ENFLOW_ERR_RANGE then raises (the outputs
                # were consumed already, so the step cannot be re-run); an
                # ENFLOW_ERR_SMALL alone (an operand entirely below 2^-7: ~1e-5
                # relative, not an overflow) warns
                _lib.defer_err(err, small_warns=True)
            else:
                _lib.check_pending()        # an older deferred word is not this launch's
                e = _lib.take_err(err)
                if _retry_fp32(e, prec):
                    # a split-precision operand left its range (an fp16 overflow, or an
                    # operand entirely below 2^-7): the step's forward again with fp32
                    # GEMMs, same inputs and draws, and the fp32 backward on its tape
                    prec = _fp32_prec(prec)
                    counts.zero_()
                    flow.forward_buffers(hw, gw, pw, vw, meta["box"], meta["r_cut"], meta["mol_ptr"],
                                         meta["max_n"], meta["noise"], ldj_mol, ldj, err, tape=tape,
                                         pair_counts=counts, prec=prec, src=src, ticket=st[1:])
                    ctx.bwd_f32 = True
                    _lib.FP32_RERUNS[0] += 1
                    e = _lib.take_err(err)
                _lib.raise_code(e)          # the reference raises inside forward
        ctx.flow, ctx.meta, ctx.kind = flow, meta, kind
        ctx.n_params = len(params)
        ctx.save_for_backward(h_in, tape, counts)
        if meta.get("per_molecule"):
            ctx.set_materialize_grads(False)
            # ArgMax's log q counts log(2 pi) once for the batch: an equal share each (dynamics.py forward)
            cst = -0.5 * math.log(2.0 * math.pi) / max(M, 1) if kind == _lib.DEQUANT_ARGMAX else 0.0
            return hw, gw, pw, vw, ldj_mol[:M] + cst
        return hw, gw, pw, vw, ldj.reshape(())

    @staticmethod
    def backward(ctx, gh, gg, gpos, gvel, gldj):
        flow, meta, kind = ctx.flow, ctx.meta, ctx.kind
        h_in, tape, counts = ctx.saved_tensors
        hid, nf, cw = flow._geometry()
        dev = h_in.device
        L = _lib.lib(nf)
        A = h_in.shape[0]
        M = meta["mol_ptr"].numel() - 1
        n_layers = len(flow.networks)
        per_mol = bool(meta.get("per_molecule"))
        if per_mol and all(t is None for t in (gh, gg, gpos, gvel, gldj)):
            return (None,) * (6 + ctx.n_params)
        if flow._params_key(dev) != ctx.train_key:      # before anything is launched
            raise RuntimeError("enflow_amd: a parameter of the flow was modified in place between forward "
                               "and backward (autograd would report a version mismatch here)")

        # private copies: the kernels turn them into the input adjoints in place
        ah, ag = _adj(gh, (A, nf), dev, clone=True), _adj(gg, (A, nf), dev, clone=True)
        apos, avel = _adj(gpos, (A, 3), dev, clone=True), _adj(gvel, (A, 3), dev, clone=True)
        if per_mol:
            # d ldj_mol [num_mols] -> one value per atom, the form the kernels read (the
            # buffer is torch's: no workspace size changes)
            amol = _adj(gldj if M else None, (max(M, 1),), dev)
            aldj = torch.empty(max(A, 1), dtype=torch.float32, device=dev)
            _lib.check(L.enflow_ldj_mol_to_atoms_f32(M, A, _lib.ptr(meta["mol_ptr"]), _lib.ptr(amol), _lib.ptr(aldj),
                                                     _lib.stream_ptr(dev)), "enflow_ldj_mol_to_atoms_f32")
        else:
            aldj = _adj(gldj, (), dev, clone=True).reshape(1)
        fwd, bwd, raw = ctx.train_bufs
        grad_layers = torch.empty_like(raw)
        dq_raw, grad_dq = None, None
        if kind == _lib.DEQUANT_ARGMAX:
            dq_raw = ctx.dq_raw
            grad_dq = torch.empty_like(dq_raw)
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        kindv = (kind | (_lib.EGCL_VARIANTS if flow._has_variants() else 0) | (_lib.BWD_F32 if ctx.bwd_f32 else 0) |
                 (_lib.BWD_LDJ_ATOMS if per_mol else 0))
        if meta["large"]:
            # the forward counted each layer's pair rows on the device: size the
            # workspace by their maximum (one small read; large systems only)
            prb = int(counts[:max(n_layers, 1)].max().item()) if n_layers else 0
            wsb = L.enflow_lf_backward_large_workspace_size(M, A, meta["max_n"], nf, hid, prb)
            ws = _alloc_ws(wsb, "enflow_lf_backward_large_workspace_size rejected the batch", dev)
            _lib.check(L.enflow_lf_backward_large_f32(
                M, A, meta["max_n"], nf, hid, _lib.ptr(meta["mol_ptr"]), _lib.ptr(meta["r_cut"]),
                _lib.ptr(meta["box"]), _lib.ptr(tape), _lib.ptr(fwd), _lib.ptr(bwd), _lib.ptr(raw), n_layers,
                kindv, _lib.ptr(dq_raw), _lib.ptr(h_in), _lib.ptr(meta["noise"]), float(flow.dt), cw,
                _lib.ptr(ah), _lib.ptr(ag), _lib.ptr(apos), _lib.ptr(avel), _lib.ptr(aldj),
                _lib.ptr(grad_layers), _lib.ptr(grad_dq), _lib.ptr(ws), wsb, prb, _lib.ptr(err),
                _lib.stream_ptr(dev)), "enflow_lf_backward_large_f32")
        else:
            prb = meta["pair_row_bound"]
            wsb = L.enflow_lf_backward_workspace_size(M, A, nf, hid, n_layers, prb)
            if os.environ.get("ENFLOW_BWD_MIN_WS") == "1":     # memory-lean: two rotating buffers
                wsb = L.enflow_lf_backward_workspace_size_min(M, A, nf, hid, n_layers, prb)
            try:
                ws = _alloc_ws(wsb, "enflow_lf_backward_workspace_size rejected the batch", dev)
            except torch.cuda.OutOfMemoryError:
                # three rotating pair-row buffers do not fit: two (the layer chain
                # then waits for the weight-gradient pass two layers up); the failed
                # request's cached blocks are released first
                torch.cuda.empty_cache()
                wsb = L.enflow_lf_backward_workspace_size_min(M, A, nf, hid, n_layers, prb)
                try:
                    ws = _alloc_ws(wsb, "enflow_lf_backward_workspace_size_min rejected the batch", dev)
                except torch.cuda.OutOfMemoryError as exc:
                    raise torch.cuda.OutOfMemoryError(
                        f"enflow_amd backward workspace ({wsb / 2**30:.2f} GiB with two rotating pair-row "
                        "buffers, the ENFLOW_BWD_MIN_WS=1 size) does not fit: train on a smaller batch") from exc
            _lib.check(L.enflow_lf_backward_f32(
                M, A, meta["max_n"], nf, hid, _lib.ptr(meta["mol_ptr"]), _lib.ptr(meta["r_cut"]),
                _lib.ptr(meta["box"]), _lib.ptr(tape), _lib.ptr(counts), _lib.ptr(fwd), _lib.ptr(bwd),
                _lib.ptr(raw), n_layers, kindv, _lib.ptr(dq_raw), _lib.ptr(h_in), _lib.ptr(meta["noise"]),
                float(flow.dt), cw, _lib.ptr(ah), _lib.ptr(ag), _lib.ptr(apos), _lib.ptr(avel), _lib.ptr(aldj),
                _lib.ptr(grad_layers), _lib.ptr(grad_dq), _lib.ptr(ws), wsb, prb, _lib.ptr(err),
                _lib.stream_ptr(dev)), "enflow_lf_backward_f32")
        if meta["check_errors"]:
            # the forward's deferred word (the reference's IndexError), read once the
            # backward is queued behind it, so the device never drains while the host
            # prepares the backward; raised before any gradient is returned (the
            # backward kernels validate their own geometry and only compute on a
            # failed batch's state).  The backward's own word is read at the next check.
            _lib.check_pending()
            _lib.defer_err(err)
        # split the flat gradients into the parameters' shapes (inputs order)
        grads = []
        rstride = grad_layers.numel() // max(len(flow.networks), 1)
        for li, net in enumerate(flow.networks):
            grads += layer_grads(net, grad_layers[li * rstride:(li + 1) * rstride])
        if kind == _lib.DEQUANT_ARGMAX:
            am = flow.dequantize
            grads += argmax_grads(am, grad_dq, am.pad_geom(hid))
        # d h of the data only exists without a learned dequantiser (z = h + noise)
        gh_in = ah if kind != _lib.DEQUANT_ARGMAX else None
        return (None, None, gh_in, ag, apos, avel) + tuple(grads)


def flow_forward_train(flow, data, noise, check_errors, per_molecule=False):
    """Differentiable LFIntegrator.forward (HIP forward with tape); per_molecule:
    LFIntegrator.forward_grad, the [num_mols] log|detJ| in the scalar's place."""
    flow._check_trainable()
    s = flow._state(data)
    dev = s["dev"]
    kind = flow._dequant_kind()
    if noise is None:
        if kind != _lib.DEQUANT_NONE:
            noise = _host_noise(kind, s["h"].shape, dev)
    else:
        noise = noise.to(device=dev, dtype=torch.float32).contiguous()
    large = s["max_n"] > _lib.TRAIN_MAX_ATOMS   # past the fused backward: large-system training kernels
    meta = dict(box=s["box"], r_cut=s["r_cut"], mol_ptr=s["mol_ptr"], max_n=s["max_n"], noise=noise,
                check_errors=check_errors, large=large, per_molecule=per_molecule,
                pair_row_bound=0 if large else pair_row_bound(data.N))
    return _write_back(data, *_apply_to_data(_FlowFunction, flow, meta, data, dev, dequantize=True))


class _ReverseFunction(torch.autograd.Function):
    """The continuous layers of LFIntegrator.reverse (dynamics.py:26-34) with the
    HIP backward.  Under autograd the reverse runs one layer per launch (the
    existing reverse entries on that layer's packed weights, dequantiser NONE),
    each launch writing its slot of the state tape (h', g', x', v') and its Q
    sums; the backward is enflow_lf_reverse_backward_f32 on that tape.  Returns
    (h, g, pos, vel, rev_ldj [num_mols]) before the dequantiser's reverse."""

    @staticmethod
    def forward(ctx, flow, meta, h, g, pos, vel, *params):
        from .dynamics import _LaunchCfg
        hid, nf, cw = flow._geometry()
        dev = h.device
        L = _lib.lib(nf)
        n_layers = len(flow.networks)
        A = h.shape[0]
        M = meta["mol_ptr"].numel() - 1
        src = tuple(t.detach().contiguous() for t in (h, g, pos, vel))
        prec = _tape_prec(flow)
        ctx.train_bufs = flow.training_layers(dev)
        ctx.train_key = flow._params_key(dev)
        fwd = ctx.train_bufs[0]
        stride = L.enflow_egcl_packed_size(hid, nf)
        # the state tape: slot l is what layer l's step leaves (the input of layer l - 1's)
        tape = tuple(torch.empty((max(n_layers, 1),) + tuple(t.shape), dtype=torch.float32, device=dev) for t in src)
        ldj_l = torch.zeros((max(n_layers, 1), max(M, 1)), dtype=torch.float32, device=dev)
        tot = torch.empty(1, dtype=torch.float32, device=dev)     # the large-system entry's batch total (unused)
        w = _lib.infer_words(dev, M, A)
        words = torch.zeros(2, dtype=torch.int32, device=dev)     # error word, ArgMax index maximum (unused)
        err = words[:1]
        large = _lib.is_large(meta["max_n"])

        def run(prec):
            cur = src
            for l in reversed(range(n_layers)):
                # the whole-workgroup instances only: a latency split is an inference choice
                cfg = _LaunchCfg(str(dev), hid, nf, cw, _lib.DEQUANT_NONE, prec, fwd[l * stride:], None, 0.0, 1,
                                 float(flow.dt))
                out = tuple(t[l] for t in tape)
                flow.reverse_buffers(*out, meta["box"], meta["r_cut"], meta["mol_ptr"], meta["max_n"], w.idx,
                                     words[1:], err, src=cur, prec=prec | _lib.PREC_NO_SPLIT, cfg=cfg,
                                     ldj_mol=ldj_l[l], ldj_total=tot if large else None)
                cur = out
            return cur

        cur = run(prec)
        if meta["check_errors"]:
            _lib.check_pending()
            e = _lib.take_err(err)
            if _retry_fp32(e, prec):
                # a split-precision operand left its range: every layer again with fp32
                # GEMMs on the same inputs, and the fp32 backward on the fp32 tapes
                prec = _fp32_prec(prec)
                ldj_l.zero_()
                _lib.FP32_RERUNS[0] += 1
                cur = run(prec)
                e = _lib.take_err(err)
            _lib.raise_code(e)          # the reference raises inside reverse
        ctx.prec = prec
        ctx.flow, ctx.meta = flow, meta
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(tape[0], tape[2], tape[3])
        rev_ldj = ldj_l[:n_layers].sum(0)[:M]      # each launch wrote minus its layer's Q sums
        return tuple(t.clone() for t in cur) + (rev_ldj,)

    @staticmethod
    def backward(ctx, gh, gg, gpos, gvel, gldj):
        flow, meta = ctx.flow, ctx.meta
        n_in = 6 + sum(len(list(n.named_parameters())) for n in flow.networks)
        if all(t is None for t in (gh, gg, gpos, gvel, gldj)):
            return (None,) * n_in
        st_h, st_p, st_v = ctx.saved_tensors
        hid, nf, cw = flow._geometry()
        dev = st_h.device
        L = _lib.lib(nf)
        A = st_h.shape[1]
        M = meta["mol_ptr"].numel() - 1
        n_layers = len(flow.networks)
        adj0 = (_adj(gh, (A, nf), dev), _adj(gg, (A, nf), dev), _adj(gpos, (A, 3), dev), _adj(gvel, (A, 3), dev))
        aldj = _adj(gldj if M else None, (max(M, 1),), dev)
        if flow._params_key(dev) != ctx.train_key:
            raise RuntimeError("enflow_amd: a parameter of the flow was modified in place between reverse_grad "
                               "and backward (autograd would report a version mismatch here)")
        fwd, bwd, raw = ctx.train_bufs
        prb = meta["pair_row_bound"]
        wsb = L.enflow_lf_reverse_backward_workspace_size(M, A, meta["max_n"], nf, hid, prb)
        ws = _alloc_ws(wsb, "enflow_lf_reverse_backward_workspace_size rejected the batch", dev)
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        var = _lib.EGCL_VARIANTS if flow._has_variants() else 0

        def run(prec):
            # in place on copies: a re-run starts from the same adjoints
            a = tuple(t.clone() for t in adj0)
            grad = torch.empty_like(raw)
            f32 = (prec & 0xff) == _lib.PREC_F32
            _lib.check(L.enflow_lf_reverse_backward_f32(
                M, A, meta["max_n"], nf, hid, _lib.ptr(meta["mol_ptr"]), _lib.ptr(meta["r_cut"]),
                _lib.ptr(meta["box"]), _lib.ptr(st_h), _lib.ptr(st_p), _lib.ptr(st_v), _lib.ptr(fwd), _lib.ptr(bwd),
                _lib.ptr(raw), n_layers, var | (_lib.BWD_F32 if f32 else 0), prec & ~_lib.PREC_NO_SPLIT,
                float(flow.dt), cw, _lib.ptr(a[0]), _lib.ptr(a[1]), _lib.ptr(a[2]), _lib.ptr(a[3]), _lib.ptr(aldj),
                _lib.ptr(grad), _lib.ptr(ws), wsb, prb, _lib.ptr(err), _lib.stream_ptr(dev)),
                "enflow_lf_reverse_backward_f32")
            return a, grad

        prec = ctx.prec
        a, grad = run(prec)
        if meta["check_errors"]:
            _lib.check_pending()
            e = _lib.take_err(err)
            if _retry_fp32(e, prec):
                # a layer's f16x3 tape lost its range where the reverse's launch did not
                # flag: every tape again with fp32 GEMMs and the fp32 backward on them
                _lib.FP32_RERUNS[0] += 1
                a, grad = run(_fp32_prec(prec))
                e = _lib.take_err(err)
            _lib.raise_code(e)
        grads = []
        rstride = grad.numel() // max(n_layers, 1)
        for li, net in enumerate(flow.networks):
            grads += layer_grads(net, grad[li * rstride:(li + 1) * rstride])
        return (None, None) + a + tuple(grads)


def flow_reverse_train(flow, data, check_errors):
    """Differentiable LFIntegrator.reverse with its per-molecule log|detJ|
    (LFIntegrator.reverse_grad)."""
    _, nf, _ = flow._geometry()
    if nf is not None and nf > _lib.TRAIN_MAX_NODE_NF:
        raise NotImplementedError(f"enflow_amd trains node_nf <= {_lib.TRAIN_MAX_NODE_NF} (got {nf})")
    for n in flow.networks:
        check_trainable(n.act_fn, "LFIntegrator.reverse_grad")
    s = flow._state(data, outputs=False)
    dev = s["dev"]
    if s["src"][0].shape[1] != nf:
        raise ValueError(f"data has {s['src'][0].shape[1]} node features, the flow's layers {nf}")
    large = s["max_n"] > _lib.TRAIN_MAX_ATOMS   # past the fused backward: large-system training kernels
    N = torch.as_tensor(data.N).reshape(-1).to(torch.int64)
    # large: every layer's pair rows (each row block's pair words rounded up to 32) stay below this
    prb = (int((N * (N - 1)).sum()) + 32 * (int(N.sum()) + N.numel() + 1)) if large else pair_row_bound(N)
    meta = dict(box=s["box"], r_cut=s["r_cut"], mol_ptr=s["mol_ptr"], max_n=s["max_n"], check_errors=check_errors,
                large=large, pair_row_bound=prb)
    h, *rest = _apply_to_data(_ReverseFunction, flow, meta, data, dev)
    # ArgMax.reverse / Floor.reverse pass no gradient (argmax / floor), as in the reference's autograd
    if flow.dequantize is not None:
        h = flow.dequantize.reverse(h.detach())
    return _write_back(data, h, *rest)


class _NLLFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, nll, meta, h, g, pos, vel, ldj):
        L = _lib.lib(h.shape[1])
        dev = h.device
        M = meta["mol_ptr"].numel() - 1
        nll_mol = torch.empty((max(M, 1), 4), dtype=torch.float32, device=dev)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        ldj_t = ldj.detach().reshape(1).contiguous()
        hc, gc, pc, vc = (t.detach().contiguous() for t in (h, g, pos, vel))
        _lib.check(L.enflow_alchemical_nll_f32(M, h.shape[0], meta["max_n"], h.shape[1],
                                               _lib.ptr(meta["mol_ptr"]), _lib.ptr(hc), _lib.ptr(gc),
                                               _lib.ptr(pc), _lib.ptr(vc), _lib.ptr(ldj_t), float(nll.kBT),
                                               float(nll.softening), float(nll.z_lj), _lib.ptr(nll_mol),
                                               _lib.ptr(loss), _lib.stream_ptr(dev)), "enflow_alchemical_nll_f32")
        ctx.nll, ctx.meta = nll, meta
        ctx.save_for_backward(hc, gc, pc, vc)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, gloss):
        h, g, pos, vel = ctx.saved_tensors
        nll, meta = ctx.nll, ctx.meta
        L = _lib.lib(h.shape[1])
        dev = h.device
        M = meta["mol_ptr"].numel() - 1
        ah, ag = torch.empty_like(h), torch.empty_like(g)
        apos, avel = torch.empty_like(pos), torch.empty_like(vel)
        aldj = torch.empty(1, dtype=torch.float32, device=dev)
        gl = gloss.detach().to(torch.float32).reshape(1).contiguous()
        _lib.check(L.enflow_alchemical_nll_backward_f32(
            M, h.shape[0], meta["max_n"], h.shape[1], _lib.ptr(meta["mol_ptr"]), _lib.ptr(h), _lib.ptr(g),
            _lib.ptr(pos), _lib.ptr(vel), float(nll.kBT), float(nll.softening), _lib.ptr(gl), _lib.ptr(ah),
            _lib.ptr(ag), _lib.ptr(apos), _lib.ptr(avel), _lib.ptr(aldj), _lib.stream_ptr(dev)),
            "enflow_alchemical_nll_backward_f32")
        return None, None, ah, ag, apos, avel, aldj.reshape(())


class _MolEnergyFunction(torch.autograd.Function):
    """Alchemical_NLL.potential_grad / .per_molecule_grad: the [num_mols] values
    of ``potential`` / ``per_molecule`` (the same forward entries, bitwise) with
    a backward that takes a per-molecule upstream gradient
    (enflow_alchemical_nll_mol_backward_f32).  ldj_mol is None for the potential,
    whose only differentiable input is pos."""

    @staticmethod
    def forward(ctx, nll, meta, h, g, pos, vel, ldj_mol):
        L = _lib.lib(h.shape[1])
        dev = h.device
        ptr = meta["mol_ptr"]
        M = ptr.numel() - 1
        nll_mol = torch.empty((max(M, 1), 4), dtype=torch.float32, device=dev)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        zero = torch.zeros(1, dtype=torch.float32, device=dev)
        hc, gc, pc, vc = (t.detach().contiguous() for t in (h, g, pos, vel))
        _lib.check(L.enflow_alchemical_nll_f32(M, h.shape[0], meta["max_n"], h.shape[1], _lib.ptr(ptr),
                                               _lib.ptr(hc), _lib.ptr(gc), _lib.ptr(pc), _lib.ptr(vc),
                                               _lib.ptr(zero), float(nll.kBT), float(nll.softening),
                                               float(nll.z_lj), _lib.ptr(nll_mol), _lib.ptr(loss),
                                               _lib.stream_ptr(dev)), "enflow_alchemical_nll_f32")
        ctx.nll, ctx.meta, ctx.potential = nll, meta, ldj_mol is None
        if ldj_mol is None:
            ctx.save_for_backward(pc)
            return nll_mol[:M, 0].contiguous()
        ctx.save_for_backward(hc, gc, pc, vc)
        ldj_t = ldj_mol.detach().contiguous()
        res = torch.empty(max(M, 1), dtype=torch.float32, device=dev)
        _lib.check(L.enflow_alchemical_nll_mol_f32(M, _lib.ptr(ptr), _lib.ptr(nll_mol), _lib.ptr(ldj_t),
                                                   float(nll.kBT), float(nll.z_lj), _lib.ptr(res),
                                                   _lib.stream_ptr(dev)), "enflow_alchemical_nll_mol_f32")
        return res[:M]

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        nll, meta = ctx.nll, ctx.meta
        if ctx.potential:
            (pos,) = ctx.saved_tensors
            h = g = vel = ah = ag = avel = None
            coef = (1.0, 0.0, 0.0, 0.0)
        else:
            h, g, pos, vel = ctx.saved_tensors
            ah, ag, avel = torch.empty_like(h), torch.empty_like(g), torch.empty_like(vel)
            coef = (1.0 / float(nll.kBT), 0.5 / float(nll.kBT), 0.5, 0.5)
        dev, nf = pos.device, meta["nf"]
        M = meta["mol_ptr"].numel() - 1
        apos = torch.empty_like(pos)
        go = gout.detach().to(torch.float32).contiguous()
        _lib.check(_lib.lib(nf).enflow_alchemical_nll_mol_backward_f32(
            M, pos.shape[0], meta["max_n"], nf, _lib.ptr(meta["mol_ptr"]), _lib.ptr(h), _lib.ptr(g), _lib.ptr(pos),
            _lib.ptr(vel), float(nll.softening), _lib.ptr(go), (ctypes.c_float * 4)(*coef), _lib.ptr(ah),
            _lib.ptr(ag), _lib.ptr(apos), _lib.ptr(avel), _lib.stream_ptr(dev)),
            "enflow_alchemical_nll_mol_backward_f32")
        return None, None, ah, ag, apos, avel, (None if ctx.potential else -go)


# ---------------------------------------------------------------------------
# standalone modules: EGCL.forward (enflow/nn/egcl.py:76-92) and ArgMax.forward
# (enflow/nn/argmax.py:13-25) as autograd Functions over the HIP backward
# ---------------------------------------------------------------------------
def layer_grads(net, flat):
    """Split one layer's flat gradient (layers_raw layout at the kernel width:
    default-flag parameters in named order, then att_nn.0 weight / bias in the
    width + 1 slots) into the module's parameters, in named_parameters() order
    (the real block of each zero-padded tensor, nn/_pad.py)."""
    geom = net.pad_geom()
    g, off = unpad_grads(flat, net.raw_named(), EGCL_HDIMS, geom)
    att = [(k, p) for k, p in net.named_parameters() if k.startswith("att_nn.")]
    if att:
        ga, _ = unpad_grads(flat[off:], att, EGCL_HDIMS, geom)
        g.update(ga)
    # act_fn's own parameters (a frozen PReLU slope) get no gradient
    own = net.act_param_ids()
    return [None if id(p) in own else g[name].contiguous().to(p.dtype)
            for name, p in net.named_parameters()]


def argmax_grads(am, flat, geom):
    """ArgMax's flat gradient split into its parameters, named_parameters() order
    (None for a frozen PReLU slope, network.1)."""
    gd, _ = unpad_grads(flat, am.kernel_named(), ARGMAX_HDIMS, geom)
    return [None if k.startswith("network.1.") else gd[k].contiguous().to(p.dtype)
            for k, p in am.named_parameters()]


class _EGCLFunction(torch.autograd.Function):
    """EGCL.forward with the HIP backward: outputs from enflow_egcl_forward_f32;
    the backward regenerates the one-layer tape (message sums, pair counts) with
    the flow's forward entry (fused or large-system) and runs
    enflow_egcl_backward_f32."""

    @staticmethod
    def forward(ctx, net, meta, h, pos, *params):
        q, f, g = net._infer(h.detach(), pos.detach(), meta)
        ctx.net, ctx.meta = net, meta
        ctx.save_for_backward(net.pad_h(h.detach()), pos.detach().to(torch.float32).contiguous())
        return q, f, g

    @staticmethod
    def backward(ctx, gq, gf, gg):
        net, meta = ctx.net, ctx.meta
        h, pos = ctx.saved_tensors
        large = meta["max_n"] > _lib.TRAIN_MAX_ATOMS
        L = _lib.lib(net.kernel_nf)
        dev = h.device
        A, nf, hid = h.shape[0], net.kernel_nf, net.kernel_hidden
        M = meta["mol_ptr"].numel() - 1
        st = _lib.stream_ptr(dev)
        prec = _lib.PREC_F16X3 | (_lib.EGCL_VARIANTS if net.variant_flags() else 0)
        # the one-layer tape: layer-input state, message sums, Q; pair counts
        hw, pw = h.clone(), pos.clone()
        gw = torch.zeros_like(h)
        vw = torch.zeros_like(pos)
        tape = torch.empty(max(L.enflow_lf_tape_size_for(A, nf, hid, 1, meta["max_n"]), 1), dtype=torch.float32,
                           device=dev)
        counts = torch.zeros(max(M, 1), dtype=torch.int32, device=dev)
        ldj_mol = torch.empty(max(M, 1), dtype=torch.float32, device=dev)
        ldj = torch.empty(1, dtype=torch.float32, device=dev)
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        fwd = net.packed(dev)
        lws = _lib.large_workspace(M, A, meta["max_n"], nf, dev) if large else None

        def record(prec):
            head = (M, A, meta["max_n"], nf, hid, _lib.ptr(meta["mol_ptr"]), _lib.ptr(meta["r_cut"]),
                    _lib.ptr(meta["box"]), _lib.ptr(hw), _lib.ptr(gw), _lib.ptr(pw), _lib.ptr(vw), _lib.ptr(fwd), 1,
                    _lib.DEQUANT_NONE, None, None, 0.0, 0.0, float(net.coords_weight), _lib.ptr(ldj_mol),
                    _lib.ptr(ldj), _lib.ptr(err))
            if large:   # the large-system forward records the tape and the backward's pair rows
                fn, tail = L.enflow_lf_forward_large_f32, (prec, _lib.ptr(tape), _lib.ptr(counts), _lib.ptr(lws),
                                                           lws.numel())
            else:
                fn, tail = L.enflow_lf_forward_f32, (None, _lib.ptr(tape), _lib.ptr(counts), prec)
            _lib.check(fn(*head, *tail, st), f"{fn.__name__} (EGCL tape, gemm_precision {prec:#x})")

        record(prec)
        bwd_flags = net.variant_flags()
        e = _lib.take_err(err)
        if _retry_fp32(e, prec):
            # the f16x3 tape lost its range (overflow, or an operand entirely below
            # 2^-7): the tape again with fp32 GEMMs, and the fp32 backward on it
            bwd_flags |= _lib.BWD_F32
            hw.copy_(h), pw.copy_(pos), gw.zero_(), vw.zero_(), counts.zero_()
            _lib.FP32_RERUNS[0] += 1
            record(_fp32_prec(prec))
            e = _lib.take_err(err)
        _lib.raise_code(e)
        raw, bwd = _bwd_section(net, dev)
        if large:
            prb = int(counts[0].item())
            wsb = L.enflow_egcl_backward_large_workspace_size(M, A, meta["max_n"], nf, hid, prb)
        else:
            prb = pair_row_bound(meta["N"])
            wsb = L.enflow_egcl_backward_workspace_size(M, A, nf, hid, prb)
        ws = _alloc_ws(wsb, "enflow_egcl_backward_workspace_size rejected the batch", dev)
        aq, af, ag = _adj(gq, (A,), dev), _adj(gf, (A, 3), dev), _padded_g_adjoint(gg, A, nf, net, dev)
        dh = torch.empty((A, nf), dtype=torch.float32, device=dev)
        dpos = torch.empty((A, 3), dtype=torch.float32, device=dev)
        grad = torch.empty_like(raw)
        if large:
            _lib.check(L.enflow_egcl_backward_large_f32(
                M, A, meta["max_n"], nf, hid, _lib.ptr(meta["mol_ptr"]), _lib.ptr(meta["r_cut"]),
                _lib.ptr(meta["box"]), _lib.ptr(tape), _lib.ptr(fwd), _lib.ptr(bwd), _lib.ptr(raw),
                bwd_flags, float(net.coords_weight), _lib.ptr(aq), _lib.ptr(af), _lib.ptr(ag),
                _lib.ptr(dh), _lib.ptr(dpos), _lib.ptr(grad), _lib.ptr(ws), wsb, prb, _lib.ptr(err), st),
                "enflow_egcl_backward_large_f32")
        else:
            _lib.check(L.enflow_egcl_backward_f32(
                M, A, meta["max_n"], nf, hid, _lib.ptr(meta["mol_ptr"]), _lib.ptr(meta["r_cut"]),
                _lib.ptr(meta["box"]), _lib.ptr(tape), _lib.ptr(counts), _lib.ptr(fwd), _lib.ptr(bwd),
                _lib.ptr(raw), bwd_flags, float(net.coords_weight), _lib.ptr(aq), _lib.ptr(af),
                _lib.ptr(ag), _lib.ptr(dh), _lib.ptr(dpos), _lib.ptr(grad), _lib.ptr(ws), wsb, prb, _lib.ptr(err),
                st), "enflow_egcl_backward_f32")
        _lib.raise_on_err(err)
        return (None, None, dh[:, :net.input_nf], dpos) + tuple(layer_grads(net, grad))


def egcl_list_backward(net, h, row, col, coord_diff, gq, gf, gg, prec=_lib.PREC_F32, return_err=False, topo=None):
    """Backward of EGCL.forward on a caller-supplied edge list: the one-layer tape
    from enflow_egcl_forward_list_tape_f32 at GEMM precision `prec`, then
    enflow_egcl_backward_list_f32 on its CSR and the CSC view of it.  An f16x3
    tape that reports ERR_RANGE / ERR_SMALL is recorded again with fp32 GEMMs and
    gets the fp32 backward.  Returns (d h [n, input_nf] fp32, d coord_diff [E, 3]
    fp32 in the caller's edge order, the layer's flat gradient); return_err: also
    the first tape's error word (0: the f16x3 instances ran).  topo: the topology
    of a prepared EdgeList over row / col; its CSR and CSC are read instead of
    built, and d coord_diff comes back through its scatter, in coord_diff's dtype."""
    L = _lib.lib(net.kernel_nf)
    dev = h.device
    n, nf, hid = int(h.shape[0]), net.kernel_nf, net.kernel_hidden
    E = int(row.numel())
    st = _lib.stream_ptr(dev)
    if n == 0:   # nothing ran: every gradient is zero (the forward refused E > 0)
        out = (h.new_zeros((0, net.input_nf), dtype=torch.float32), h.new_zeros((0, 3), dtype=torch.float32),
               torch.zeros(net.kernel_raw(dev).numel() + hid + 1, device=dev))
        return out + (0,) if return_err else out
    var = _lib.EGCL_VARIANTS if net.variant_flags() else 0
    *_, e0, tape, csr = net._infer_list(h, row, col, coord_diff, prec=prec, return_err=True, tape=True, topo=topo)
    bwd_flags = net.variant_flags()
    e = e0
    if (prec & 0xff) == _lib.PREC_F32:
        bwd_flags |= _lib.BWD_F32
    elif _retry_fp32(e, prec | var):
        bwd_flags |= _lib.BWD_F32
        _lib.FP32_RERUNS[0] += 1
        *_, e, tape, csr = net._infer_list(h, row, col, coord_diff, prec=_lib.PREC_F32, return_err=True, tape=True,
                                           topo=topo)
    _lib.raise_code(e)
    row_ptr, colp, cd, order = csr
    col_ptr, col_perm = net._list_csc(n, colp) if topo is None else topo.csc()
    fwd = net.packed(dev)
    raw, bwd = _bwd_section(net, dev)
    wsb = L.enflow_egcl_backward_list_workspace_size(n, E, nf, hid)
    ws = _alloc_ws(wsb, "enflow_egcl_backward_list_workspace_size rejected the list", dev)
    aq, af, ag = _adj(gq, (n,), dev), _adj(gf, (n, 3), dev), _padded_g_adjoint(gg, n, nf, net, dev)
    dh = torch.empty((n, nf), dtype=torch.float32, device=dev)
    dcd_sorted = torch.empty((E, 3), dtype=torch.float32, device=dev)
    # returned flat to the caller: a default-flag layer's backward never writes the att_nn.0
    # slots (no descriptor for them), so they are zero here, not whatever the block held
    grad = torch.zeros_like(raw)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.check(L.enflow_egcl_backward_list_f32(
        n, E, nf, hid, _lib.ptr(row_ptr), _lib.ptr(colp), _lib.ptr(cd), _lib.ptr(col_ptr), _lib.ptr(col_perm),
        _lib.ptr(tape), _lib.ptr(fwd), _lib.ptr(bwd), _lib.ptr(raw), bwd_flags, float(net.coords_weight),
        _lib.ptr(aq), _lib.ptr(af), _lib.ptr(ag), _lib.ptr(dh), _lib.ptr(dcd_sorted), _lib.ptr(grad), _lib.ptr(ws),
        wsb, _lib.ptr(err), st), "enflow_egcl_backward_list_f32")
    _lib.raise_on_err(err)
    if topo is None:
        dcd = torch.empty_like(dcd_sorted)
        dcd[order] = dcd_sorted          # the stable sort undone: the caller's edge order
    else:
        dcd = topo.scatter(dcd_sorted, coord_diff.dtype)
    out = (dh[:, :net.input_nf], dcd, grad)
    return out + (e0,) if return_err else out


class _EGCLListFunction(torch.autograd.Function):
    """EGCL.forward on a caller-supplied edge list with the HIP backward: outputs
    from the inference call (enflow_egcl_forward_list_f32, fp32 GEMMs); the
    backward records the one-layer tape on the same list and runs
    enflow_egcl_backward_list_f32 (egcl_list_backward).  topo: the topology of a
    prepared EdgeList (None for a plain list): both directions read its arrays."""

    @staticmethod
    def forward(ctx, net, topo, row, col, h, coord_diff, *params):
        q, f, g = net._infer_list(h.detach(), row, col, coord_diff.detach(), topo=topo)
        ctx.net, ctx.topo = net, topo
        ctx.cd_dtype = coord_diff.dtype
        ctx.save_for_backward(h.detach(), row, col, coord_diff.detach())
        return q, f, g

    @staticmethod
    def backward(ctx, gq, gf, gg):
        net = ctx.net
        h, row, col, cd = ctx.saved_tensors
        dh, dcd, grad = egcl_list_backward(net, h, row, col, cd, gq, gf, gg, topo=ctx.topo)
        return (None, None, None, None, dh.to(h.dtype), dcd.to(ctx.cd_dtype)) + tuple(layer_grads(net, grad))


class _ArgMaxFunction(torch.autograd.Function):
    """ArgMax.forward with the HIP backward (enflow_argmax_backward_f32)."""

    @staticmethod
    def forward(ctx, am, meta, h, noise, *params):
        z, lq = am._infer(h.detach(), noise, meta)
        ctx.am, ctx.meta = am, meta
        ctx.save_for_backward(h.detach().to(torch.float32).contiguous(), noise)
        return z, lq

    @staticmethod
    def backward(ctx, gz, glq):
        am, meta = ctx.am, ctx.meta
        h, noise = ctx.saved_tensors
        L = _lib.lib(am.node_nf)
        dev = h.device
        A, nf, hid = h.shape[0], am.node_nf, am.kernel_hidden
        raw = am.kernel_raw(dev)
        az = (torch.zeros_like(h) if gz is None else gz.detach().to(torch.float32).contiguous())
        alq = (torch.zeros(1, device=dev) if glq is None else glq.detach().to(torch.float32).reshape(1).contiguous())
        grad = torch.empty_like(raw)
        wsb = L.enflow_argmax_backward_workspace_size(A, nf, hid)
        ws = _alloc_ws(wsb, "enflow_argmax_backward_workspace_size rejected the batch", dev)
        _lib.check(L.enflow_argmax_backward_f32(
            meta["mol_ptr"].numel() - 1, A, meta["max_n"], nf, hid, _lib.ptr(meta["mol_ptr"]), _lib.ptr(h),
            _lib.ptr(raw), _lib.ptr(noise), _lib.ptr(az), _lib.ptr(alq), _lib.ptr(grad), _lib.ptr(ws), wsb,
            _lib.stream_ptr(dev)), "enflow_argmax_backward_f32")
        grads = argmax_grads(am, grad, am.pad_geom())
        # h is the categorical data (one-hot, argmax.py:13): no gradient is returned for it
        return (None, None, None, None) + tuple(grads)
