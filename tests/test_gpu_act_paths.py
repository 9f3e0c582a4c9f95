"""act_fn other than SiLU on every path that applies or differentiates it.

flow_device.h holds one act_f and one act_d with 14 kinds; the kernels reach
them from about a dozen sites, each behind its own path (fused <= 32 atoms, the
33..64 instance, the large-system branch, the 16-feature library, the fp32
backward, standalone EGCL / ArgMax, the edge-list entry, reverse_grad,
forward_grad), and the inference kernels read the code (kind, p0, p1) at their
own offsets (narrow: L.vfl + 1; wide: L.misc + 3; ArgMax: L.act or the raw
vector's trailer).  tests/test_gpu_act.py pins the forward of every kind on the
fused path with parameters that never leave the main branch; here

1. every kind's derivative: one NLL training step per kind on the fused
   <= 32-atom path against the float64 gradient oracle;
2. the other backward paths with the parameterised kinds (PARAM);
3. the inference paths with a PARAM code in the layers and a *different*
   parameterised code in the ArgMax, so that a p0 / p1 mix-up shows.

The codes are non-default, so every parameter is live and both arms of every
branch are taken (tests/test_act_paths_host.py asserts the shares on the CPU and
pins the oracles' activations to torch's modules at these parameters).

Bars: GRAD_TOL / LOSS_TOL of tests/test_gpu_train.py for gradients and the
loss, 1e-5 normwise per output tensor and on log|detJ|.  Every case first
asserts that the same oracle evaluated in float32 on the CPU is within half of
each bar of the float64 one.  A tensor that is exactly zero in the oracle must
be exactly zero on the GPU.  The worst error per section is printed as it grows
(beside the activation table, records the measured ones).
"""
import copy
import functools

import numpy as np
import pytest
import torch
from torch import nn

from oracle import enflow_oracle as O
from oracle import enflow_oracle_grad as OG
from _fixtures import act_module, normwise, scalar_rel, worst_of, assert_all_within
from _wide import oracle_params, f32
from _edge_list_grad import case_inputs, rand_weights
from test_gpu_train import GRAD_TOL, LOSS_TOL
from test_gpu_grad_edges import _gpu_batch, _gpu_grads, _compare, _assert_f32_floor, _flat
import test_gpu_edge_list_grad as ELT
import test_gpu_reverse_grad as RGT
import test_gpu_forward_grad as FGT
from test_gpu_wide_hidden import _refs, _rev_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5
KEYS = ("h", "g", "pos", "vel")

CODES = {
    "relu": (1, 0, 0), "leaky": (2, 0.05, 0), "elu": (3, 0.7, 0), "celu": (4, 1.3, 0), "selu": (5, 0, 0),
    "gelu": (6, 0, 0), "gelutanh": (7, 0, 0), "tanh": (8, 0, 0), "sigmoid": (9, 0, 0), "softplus": (10, 1.5, 0.5),
    "mish": (11, 0, 0), "hardtanh": (12, -0.4, 0.9), "identity": (13, 0, 0),
}
# both parameters, an asymmetric pair, a divisor and the longest derivative
PARAM = ("softplus", "hardtanh", "celu", "gelutanh")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


_WORST = {}


def _record(section, err):
    """The worst error of a section so far (printed; DESIGN.md copies the last line per section)."""
    _WORST[section] = worst_of([_WORST.get(section, 0.0), err])
    print(f"[act paths] {section}: this case {err:.2e}, worst so far {_WORST[section]:.2e}")


# ---------------------------------------------------------------------------
# the model recipe of every section
# ---------------------------------------------------------------------------
def flow_model(act, dq_act, hid, nf=5):
    """Two EGCL layers with act_fn `act` -- layer 0 with attention, layer 1 with
    norm_diff and tanh -- and an ArgMax with act_fn `dq_act` (names of CODES),
    weights from torch.manual_seed(3), on the CPU.  (EGCL(tanh=True) holds a
    non-leaf tensor, so a model is built again from the seed, not deep-copied.)"""
    from enflow_amd.nn import EGCL, ArgMax
    from enflow_amd.flow import LFIntegrator
    from enflow_amd.data.synthetic import default_dt
    torch.manual_seed(3)
    nets = [EGCL(nf, nf, hid, act_fn=act_module(CODES[act]), attention=True),
            EGCL(nf, nf, hid, act_fn=act_module(CODES[act]), norm_diff=True, tanh=True)]
    return LFIntegrator(nets, ArgMax(nf, hid, act_fn=act_module(CODES[dq_act])), dt=default_dt())


def grad_dicts(model):
    """The gradient oracle's layer dicts (with "act" and "flags") and dequantiser dict (with "act")."""
    layers = []
    for n in model.networks:
        p = {k: v.detach().double().numpy() for k, v in n.named_parameters()}
        p["act"] = tuple(float(x) for x in n.act())
        p["flags"] = (bool(n.attention), bool(n.norm_diff), bool(n.tanh))
        layers.append(p)
    dq = {k: v.detach().double().numpy() for k, v in model.dequantize.named_parameters()}
    dq["act"] = tuple(float(x) for x in model.dequantize.act())
    return layers, dq


# id -> (sizes, make_molecules keywords, hidden_nf, node features, data seed).
#
# The data seeds are chosen for the float32 floor.  The one-element gradient of att_nn.0.bias (and the
# other small coord_nn / att_nn tensors) is a sum over every edge that nearly cancels on some batches,
# and the float32 oracle's error on it then depends on the CPU's float32 libm and BLAS: with seed 7 the
# floor of GELU on p0.att_nn.0.bias was 7.4e-7 on one machine and 3.1e-5 (past half the bar) on another,
# and CELU(1.3) on bound64 gave 4.9e-5.  So each seed was taken where the float32 oracle stays small under
# rounding-sized changes as well: five runs with every weight scaled by 1 + 6e-8 N(0, 1), each against
# the float64 oracle of the unchanged weights, worst tensor of the worst kind: fused 3.0e-6 (seed 7:
# 5.3e-5), bound64 3.0e-6, large65 3.7e-6, nf16 1.3e-6
TRAIN_CASES = {
    "fused": ([22, 9, 2], {}, 32, 5, 14),
    "bound64": ([33, 64, 2], dict(radius=5.7), 32, 5, 9),
    "large65": ([65, 1, 22], dict(radius=5.7), 32, 5, 10),
    "nf16": ([22, 9], {}, 32, 16, 7),
}


@functools.lru_cache(maxsize=None)
def train_setup(act, case):
    """Batch (float32-representable), noise and the oracle's dicts of one NLL training step."""
    from enflow_amd import _lib
    from enflow_amd.data.synthetic import make_molecules
    sizes, kw, hid, nf, seed = TRAIN_CASES[case]
    b = f32(make_molecules(len(sizes), sizes, nf=nf, seed=seed, **kw))
    max_n = int(np.diff(b["mol_ptr"]).max())
    if case == "bound64":
        assert max_n == 64 == _lib.TRAIN_MAX_ATOMS
    elif case == "large65":
        assert max_n > _lib.TRAIN_MAX_ATOMS
    else:
        assert max_n <= 32
    model = flow_model(act, act, hid, nf)
    eps = np.random.default_rng(13).normal(size=b["h"].shape).astype(np.float32)
    layers, dq = grad_dicts(model)
    return dict(b=b, eps=eps, layers=layers, dq=dq, dt=float(model.dt), hid=hid, nf=nf)


def oracle_step(s, dtype):
    """(loss, flat gradients) of the gradient oracle's training step in `dtype`."""
    from enflow_amd.data.synthetic import default_kBT
    loss, _, gl, gd, _, gi = OG.train_loss_and_grads(s["layers"], s["dq"], s["b"], s["eps"].astype(np.float64), s["dt"],
                                                     default_kBT(), 0.1, dtype=dtype, input_grads=True)
    return loss, _flat(gl, gd, gi)


@functools.lru_cache(maxsize=None)
def train_ref(act, case):
    """((loss, grads) float64, the float32-oracle floor); cached, never modified."""
    s = train_setup(act, case)
    r64, r32 = oracle_step(s, torch.float64), oracle_step(s, torch.float32)
    return r64, _assert_f32_floor(f"{act}-{case}", r64, r32)


def _train_vs_oracle(section, act, case, prec):
    from enflow_amd.flow import Alchemical_NLL
    from enflow_amd.data.synthetic import default_kBT
    s = train_setup(act, case)
    ref, floor = train_ref(act, case)
    model = flow_model(act, act, s["hid"], s["nf"]).cuda()
    model.gemm_precision = prec
    data, leaves = _gpu_batch(s["b"])
    out, ldj = model(data, noise=torch.tensor(s["eps"], device="cuda"))
    loss = Alchemical_NLL(kBT=default_kBT(), softening=0.1)(out, ldj)
    loss.backward()
    got = _gpu_grads(model, leaves)
    _record(section, worst_of({k: normwise(got[k], v) for k, v in ref[1].items() if np.any(v)}))
    _compare(f"{act}-{case}-{prec}", float(loss.detach()), got, ref, floor)


# ---------------------------------------------------------------------------
# 1. every derivative: one NLL training step per kind, fused <= 32 atoms
# ---------------------------------------------------------------------------
S1 = [(a, "f16x3") for a in CODES] + [(a, "f32") for a in PARAM]


@pytest.mark.parametrize("act,prec", S1, ids=["-".join(p) for p in S1])
def test_training_step_every_kind(act, prec):
    """Loss, every parameter gradient, the ArgMax gradients and d g / d pos / d vel
    of [22, 9, 2] atoms at hidden 32: act_d of the kind on the fused backward
    (f32: the ENFLOW_BWD_F32 backward)."""
    _train_vs_oracle("1 every kind, fused", act, "fused", prec)


# ---------------------------------------------------------------------------
# 2. the other backward paths with the parameterised kinds
# ---------------------------------------------------------------------------
S2 = ([(a, c) for c in ("bound64", "large65") for a in PARAM] + [(a, "nf16") for a in ("softplus", "hardtanh")])


@pytest.mark.parametrize("act,case", S2, ids=["-".join(p) for p in S2])
def test_training_step_other_instances(act, case):
    """bound64: the 33..64-atom instance; large65: the large-system backward past
    TRAIN_MAX_ATOMS; nf16: the 16-feature library."""
    _train_vs_oracle(f"2 {case}", act, case, "f16x3")


STANDALONE = ["relu", "celu", "selu", "gelutanh", "sigmoid", "hardtanh", "identity", "softplus"]


@functools.lru_cache(maxsize=None)
def standalone_ref(act):
    """tests/test_gpu_act.py::test_standalone_modules_backward_with_activation's
    construction on the CPU: (batch, EGCL, ArgMax, adjoints, noise, float64
    gradients) after the float32 floor.  The noise comes from numpy, so that the
    reference needs no GPU."""
    from enflow_amd.nn import EGCL, ArgMax
    from enflow_amd.data.synthetic import make_molecules
    code = tuple(float(x) for x in CODES[act])
    b = f32(make_molecules(3, [22, 9, 15], nf=5, seed=40))
    torch.manual_seed(41)
    net = EGCL(5, 5, 64, act_fn=act_module(code))
    torch.manual_seed(43)
    am = ArgMax(5, 32, act_fn=act_module(code))
    rng = np.random.default_rng(42)
    n = b["h"].shape[0]
    w = {k: rng.normal(size=s).astype(np.float32) for k, s in (("q", (n, 1)), ("f", (n, 3)), ("g", (n, 5)))}
    w["z"] = rng.normal(size=(n, 5)).astype(np.float32)
    eps = np.random.default_rng(44).normal(size=(n, 5)).astype(np.float32)
    row, col, eb = O.batch_edges(b["pos"], b["box"], b["r_cut"], b["mol_ptr"])
    res = []
    for dtype in (torch.float64, torch.float32):
        t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64)).to(dtype)  # noqa: E731
        P = {k: t(v.detach().numpy()).requires_grad_(True) for k, v in net.named_parameters()}
        h, pos = t(b["h"]).requires_grad_(True), t(b["pos"]).requires_grad_(True)
        q, f, g = OG._egcl(P, h, pos, torch.as_tensor(row), torch.as_tensor(col), t(eb), n, 1.0, act=code)
        loss = (q * t(w["q"])).sum() + (f * t(w["f"])).sum() + (g * t(w["g"])).sum()
        loss.backward()
        grads = {k: v.grad.double().numpy() for k, v in P.items()}
        grads.update({"in.h": h.grad.double().numpy(), "in.pos": pos.grad.double().numpy()})
        D = {k: t(v.detach().numpy()).requires_grad_(True) for k, v in am.named_parameters()}
        z, lq = OG._argmax(D, t(b["h"]), t(eps), code)
        dloss = (z * t(w["z"])).sum() + 0.7 * lq
        dloss.backward()
        grads.update({f"dq.{k}": v.grad.double().numpy() for k, v in D.items()})
        res.append((float(loss.detach()) + float(dloss.detach()), grads))
    return b, net, am, w, eps, res[0], _assert_f32_floor(f"standalone {act}", *res)


@pytest.mark.parametrize("act", STANDALONE)
def test_standalone_modules_backward(act):
    """EGCL.forward and ArgMax.forward trained directly: the kinds whose
    derivative test_standalone_modules_backward_with_activation does not run,
    and softplus across its threshold."""
    from enflow_amd.data import Data
    b, net, am, w, eps, ref, floor = standalone_ref(act)
    gnet, gam = copy.deepcopy(net).to(DEV), copy.deepcopy(am).to(DEV)
    t32 = lambda a: torch.tensor(a, dtype=torch.float32, device=DEV)  # noqa: E731
    d = Data.from_arrays(b, device=DEV)
    h = d.h.clone().requires_grad_(True)
    pos = d.pos.clone().requires_grad_(True)
    d.pos = pos
    q, f, g = gnet(h, d.edges)
    loss = (q * t32(w["q"])).sum() + (f * t32(w["f"])).sum() + (g * t32(w["g"])).sum()
    loss.backward()
    z, lq = gam(t32(b["h"]), noise=t32(eps))
    dloss = (z * t32(w["z"])).sum() + 0.7 * lq
    dloss.backward()
    torch.cuda.synchronize()
    got = {k: p.grad.double().cpu().numpy() for k, p in gnet.named_parameters()}
    got.update({"in.h": h.grad.double().cpu().numpy(), "in.pos": pos.grad.double().cpu().numpy()})
    got.update({f"dq.{k}": p.grad.double().cpu().numpy() for k, p in gam.named_parameters()})
    _record("2 standalone", worst_of({k: normwise(got[k], v) for k, v in ref[1].items() if np.any(v)}))
    _compare(f"standalone {act}", float(loss.detach()) + float(dloss.detach()), got, ref, floor)


@pytest.mark.parametrize("act", ["hardtanh", "softplus"])
def test_edge_list_backward(act):
    """EGCL on a caller-supplied list (lf_layer_bwd_kernel<.., LIST>): the random_20
    case of tests/test_gpu_edge_list_grad.py."""
    net = ELT.module(7, act_fn=act_module(CODES[act]))
    n, row, col, cd, h = case_inputs("random_20", net.input_nf)
    w = rand_weights(n, net.output_nf)
    ref = ELT.reference(net, h, row, col, cd, w, f"random_20 {act}")
    got = ELT.run(net, h, row, col, cd, w, itype=torch.int32)
    _record("2 edge list", ELT.compare(f"random_20 {act}", got, ref))


def _hardtanh():
    return nn.Hardtanh(-0.4, 0.9)


def _softplus():
    return nn.Softplus(1.5, 0.5)


# the cases of tests/test_gpu_reverse_grad.py / test_gpu_forward_grad.py with a parameterised act_fn, under
# names of their own in those modules' tables (their builders, references and comparisons then apply as they are)
RGT.CASES.setdefault("act_hardtanh_fused", (lambda: RGT._model(RGT._egcl(2, 5, 32, 11, act_fn=_hardtanh())),
                                            lambda: RGT._batch([5, 9, 22], seed=12), "hgpvl"))
RGT.CASES.setdefault("act_hardtanh_n70_chain", (lambda: RGT._model(RGT._egcl(2, 5, 32, 81, act_fn=_hardtanh())),
                                                lambda: RGT._batch([70, 22], seed=82, chain=True), "hgpvl"))
FGT.CASES.setdefault("act_softplus_variants",
                     (lambda: FGT._model("none", hid=64, seed=61, attention=True, norm_diff=True, tanh=True,
                                         act_fn=_softplus()), lambda: FGT._batch([9, 22], seed=62)))
FGT.CASES.setdefault("act_softplus_n70", (lambda: FGT._model("argmax", seed=41, act_fn=_softplus()),
                                          lambda: FGT._batch([70, 22], seed=42)))


@pytest.mark.parametrize("name", ["act_hardtanh_fused", "act_hardtanh_n70_chain"])
def test_reverse_grad_hardtanh(name):
    """LFIntegrator.reverse_grad (the reverse_grad glue; n70_chain: its large-system branch)."""
    model, b, use = RGT._build(name)
    w = RGT._weights(b, use)
    ref = RGT._reference(name, RGT.RG.model_layers(model), b, float(model.dt), w)
    _, _, vals, gi, gl = RGT._run_gpu(model, b, w)
    errs, gerr = RGT._compare(name, ref, use, vals, gi, gl)
    _record("2 reverse_grad", worst_of(gerr))


@pytest.mark.parametrize("name", ["act_softplus_variants", "act_softplus_n70"])
def test_forward_grad_softplus(name):
    """LFIntegrator.forward_grad (the per-atom log|detJ| translation unit; n70: its BIG row blocks)."""
    model, b, noise, kind = FGT._build(name)
    ref, S = FGT._reference(name)
    w, c = FGT._upstream(b, kind)
    vals, g, _ = FGT._run(model, b, noise, w, c)
    _record("2 forward_grad", worst_of({k: normwise(g[k], r) for k, r in ref.items()
                                        if not (k.startswith("out.") or k == "ldj_mol") and np.any(r)}))
    FGT._compare(name, ref, S, vals, g)


# ---------------------------------------------------------------------------
# 3. inference paths that read the code at their own offsets
# ---------------------------------------------------------------------------
def dq_act_for(act):
    """A parameterised ArgMax code that differs from the layers': ELU(0.7) beside
    softplus layers, Softplus(1.5, 0.5) beside the others."""
    return "elu" if act == "softplus" else "softplus"


def _chain(sizes, seed):
    from enflow_amd.data.synthetic import make_molecules
    return f32(make_molecules(len(sizes), sizes, nf=5, seed=seed, chain=True))


def _walk(sizes, seed):
    from enflow_amd.data.synthetic import make_molecules
    return f32(make_molecules(len(sizes), sizes, nf=5, seed=seed))


# id -> (batch, hidden_nf); each the smallest shape that selects its path
INFER = {
    "rowblocked": (lambda: _chain([70, 40], 37), 64),     # the row-blocked 65..256 instance
    "large257": (lambda: _chain([257], 35), 32),          # the large-system kernels
    "wide160": (lambda: _walk([40, 22], 35), 160),        # enflow_wide.hip, padded to 256
    "wide256": (lambda: _walk([40, 22], 37), 256),
    "ahead": (lambda: _walk([22, 9, 31], 35), 128),       # test_argmax_ahead_of_the_flow_hardtanh
}
_FLOW_REF = {}


def flow_ref(case, act, dq_act):
    """(batch, noise, oracle forward, its log|detJ|, the float32-rounded forward
    output, oracle reverse of that) of an inference case, after the float32
    floors of tests/test_gpu_wide_hidden.py (_refs, _rev_ref: half of 1e-5 per
    tensor and on log|detJ|).  Cached, never modified; the noise is numpy's, so
    the reference needs no GPU."""
    key = (case, act, dq_act)
    if key not in _FLOW_REF:
        mk, hid = INFER[case]
        b = mk()
        model = flow_model(act, dq_act, hid)
        eps = np.random.default_rng(5).normal(size=b["h"].shape).astype(np.float32)
        ref, ref_ldj = _refs(model, b, eps.astype(np.float64), "argmax")
        st = f32({**ref, "box": b["box"], "r_cut": b["r_cut"]})
        st["mol_ptr"] = b["mol_ptr"]
        _FLOW_REF[key] = (b, eps, ref, ref_ldj, st, _rev_ref(model, st, "none"))
    return _FLOW_REF[key]


def _flow_vs_oracle(section, case, act, dq_act, prec):
    """Forward, and reverse of the oracle's float32-rounded forward output, on
    the GPU against flow_ref; no fp32 re-run; the dequantised h exact."""
    from enflow_amd import _lib
    from enflow_amd.data import Data
    b, eps, ref, ref_ldj, st, rref = flow_ref(case, act, dq_act)
    model = flow_model(act, dq_act, INFER[case][1]).to(DEV)
    model.gemm_precision = prec
    r0 = _lib.FP32_RERUNS[0]
    with torch.no_grad():
        out, ldj = model(Data.from_arrays(b, device=DEV), noise=torch.tensor(eps, device=DEV))
        back = model.reverse(Data.from_arrays(st, device=DEV))
    assert _lib.FP32_RERUNS[0] == r0, "the forward was re-run in fp32"
    errs = {k: normwise(getattr(out, k).cpu().numpy(), ref[k]) for k in KEYS}
    errs["ldj"] = scalar_rel(float(ldj), ref_ldj)
    errs.update({"rev_" + k: normwise(getattr(back, k).cpu().numpy(), rref[k]) for k in ("g", "pos", "vel")})
    print(f"{case} {act} / ArgMax {dq_act} {prec}:", {k: f"{v:.2e}" for k, v in errs.items()})
    _record(section, worst_of(errs))
    hb, want = back.h.cpu().numpy(), O.argmax_reverse(rref["h"])
    assert hb.shape == want.shape and np.array_equal(hb, want)
    assert_all_within(errs, TOL, f"{case} {act} {prec}")
    return model, out, ldj


S3 = [(c, a, p) for c in ("rowblocked", "large257", "wide160", "wide256") for a in PARAM for p in ("f16x3", "f32")]


@pytest.mark.parametrize("case,act,prec", S3, ids=["-".join(p) for p in S3])
def test_inference_paths(case, act, prec):
    """rowblocked: chains of [70, 40] atoms at hidden 64 (narrow kernels, the code
    at L.vfl + 1); large257: one 257-atom chain at hidden 32; wide160 / wide256:
    enflow_wide.hip (the code at L.misc + 3, packed by wide_pack_kernel)."""
    from enflow_amd import _lib
    b, hid = flow_ref(case, act, dq_act_for(act))[0], INFER[case][1]
    max_n = int(np.diff(b["mol_ptr"]).max())
    if case == "rowblocked":
        assert max_n == 70 and not _lib.is_large(70)
    elif case == "large257":
        assert max_n == 257 and _lib.is_large(257)
    model, _, _ = _flow_vs_oracle(f"3 {case}", case, act, dq_act_for(act), prec)
    assert all(n.wide == (hid > 128) for n in model.networks)


def test_wide_argmax_alone_softplus():
    """ArgMax(5, 256, act_fn=Softplus(1.5, 0.5)) on 71 atoms (wide_argmax_kernel)."""
    from enflow_amd.nn import ArgMax
    torch.manual_seed(88)
    am = ArgMax(5, 256, act_fn=_softplus()).to(DEV)
    assert tuple(am.act()) == (10, 1.5, 0.5)
    hq = np.eye(5)[np.random.default_rng(9).integers(0, 5, size=71)]
    eps = np.random.default_rng(10).normal(size=(71, 5)).astype(np.float32)
    z64, lq64 = O.argmax_forward(oracle_params(am), hq, eps.astype(np.float64))
    z32, lq32 = O.argmax_forward(oracle_params(am, np.float32), hq.astype(np.float32), eps)
    assert normwise(z32, z64) <= TOL / 2 and scalar_rel(lq32, lq64) <= TOL / 2
    with torch.no_grad():
        z, lq = am(torch.tensor(hq, dtype=torch.float32, device=DEV), noise=torch.tensor(eps, device=DEV))
    errs = {"z": normwise(z.cpu().numpy(), z64), "log_q": scalar_rel(float(lq), lq64)}
    _record("3 wide ArgMax alone", worst_of(errs))
    assert_all_within(errs, TOL, "ArgMax(5, 256, Softplus(1.5, 0.5))")


def _forward_with_ahead(model, d, eps, ahead):
    from enflow_amd import _lib
    prev = _lib.set_dequant_ahead(ahead)
    try:
        with _lib.KernelTimer() as t, torch.no_grad():
            o, ldj = model(d.clone(), noise=eps)
    finally:
        _lib.set_dequant_ahead(True if prev is None else bool(prev))
    return o, ldj, set(t.stats)


def test_argmax_ahead_of_the_flow_hardtanh():
    """ArgMax Hardtanh(-0.4, 0.9) ahead of the flow (dequant_kernel) against the
    dequantisation fused into the flow kernel, hidden 128, softplus layers.

    The ahead kernel engages only for batches of more molecules than the device
    has CUs (tests/test_gpu_dequant.py), so the batch [22, 9, 31] alone runs the
    fused form under either setting: it is compared with the oracle, and its two
    runs bitwise.  The same three molecules repeated past the CU count do
    launch dequant_kernel: ahead and fused are then bitwise equal on the outputs
    (log|detJ| within 1e-6: its sum order differs), and the first three
    molecules, which do not interact with the copies, meet the oracle's bar."""
    from enflow_amd.data import Data
    b, eps, ref, _, _, _ = flow_ref("ahead", "softplus", "hardtanh")
    model, out, ldj = _flow_vs_oracle("3 ArgMax ahead", "ahead", "softplus", "hardtanh", "f16x3")
    d = Data.from_arrays(b, device=DEV)
    A = d.h.shape[0]
    et = torch.tensor(eps, device=DEV)
    o1, l1, k1 = _forward_with_ahead(model, d, et, True)
    o0, l0, k0 = _forward_with_ahead(model, d, et, False)
    assert "dequant_kernel" not in k1 and "dequant_kernel" not in k0, (k1, k0)
    for k in KEYS:
        assert torch.equal(getattr(o1, k), getattr(o0, k)) and torch.equal(getattr(o1, k), getattr(out, k)), k
    assert float(l1) == float(l0) == float(ldj)
    # past the CU count
    reps = torch.cuda.get_device_properties(0).multi_processor_count // 3 + 1
    tiled = {k: np.concatenate([b[k]] * reps) for k in KEYS + ("box", "r_cut")}
    tiled["mol_ptr"] = np.concatenate([[0], np.cumsum(np.tile(np.diff(b["mol_ptr"]), reps))]).astype(np.int64)
    dt = Data.from_arrays(tiled, device=DEV)
    et = et.repeat(reps, 1)
    o1, l1, k1 = _forward_with_ahead(model, dt, et, True)
    o0, l0, k0 = _forward_with_ahead(model, dt, et, False)
    assert "dequant_kernel" in k1 and "dequant_kernel" not in k0, (k1, k0)
    for k in KEYS:
        assert torch.equal(getattr(o1, k), getattr(o0, k)), k
    assert abs(float(l1) - float(l0)) <= 1e-6 * abs(float(l0))
    errs = {k: normwise(getattr(o1, k)[:A].cpu().numpy(), ref[k]) for k in KEYS}
    _record("3 ArgMax ahead", worst_of(errs))
    assert_all_within(errs, TOL, "dequant_kernel with Hardtanh(-0.4, 0.9) vs the oracle")


