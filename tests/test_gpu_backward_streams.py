"""The auxiliary-stream protocol of the training backward (AuxPipe in
enflow_backward.hip): layer l's weight-gradient pass runs on a second stream and
reads pair-row buffer l % depth while the layer chain writes the others, so a
wrong wait is a race on a buffer that is only reused when the chain is deeper
than the rotation.  Shapes at which every loop wraps:

  fused         H 32, nf 5, 5 layers, molecules of [3, 22, 33] atoms: three buffers, wrap at layer 1
  fused_min_ws  the same under ENFLOW_BWD_MIN_WS=1: two buffers, wrap at layer 2
  large         a 65-atom molecule beside a 3-atom one, 3 layers: two buffers, wrap at layer 0
  list          the standalone backward on a 40-node, 200-edge list (the one-layer case)

(a) every parameter gradient and input adjoint of a default run equals, bitwise,
    that of a run under ENFLOW_SERIAL_BWD=1 (the layer chain waits for each
    weight-gradient pass: no overlap, nothing to race with);
(b) the per-kernel launch counts of one backward (_lib.KernelTimer) equal the
    counts COUNTS below, recorded on an MI355X from the library before its host
    half was rewritten around BwdCall / AuxPipe.  Per layer: one layer backward,
    one outer_x3 and one atom-row outer_acc launch and their reduction; the
    ArgMax dequantiser adds one outer_acc and one reduction.  Recorded there:
      fused, fused_min_ws  lf_layer_bwd 5, outer_x3 5, outer_acc 6, reduce_part 6, nll_bwd 1
      large                lf_layer_bwd 3, lg_idmap / lg_images / lg_pairs / lg_bwd_offsets /
                           lg_colsum / lg_colfinal 3 each, outer_x3 3, outer_acc 4, reduce_part 4, nll_bwd 1
      list                 el_layer_tape 1, el_bwd_offsets 1, lf_layer_bwd_list 1, el_colsum 1,
                           outer_x3 1, outer_acc 1, reduce_part 1
    The rewritten library gave the same counts and both assertions held on either.
"""
import numpy as np
import pytest
import torch

from _edge_list_grad import List, rand_cd, rand_weights, weighted

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

_FUSED = {"lf_layer_bwd_kernel": 5, "nll_bwd_kernel": 1, "outer_acc_kernel": 6, "outer_x3_kernel": 5,
          "reduce_part_kernel": 6}
COUNTS = {
    "fused": _FUSED,
    "fused_min_ws": _FUSED,
    # per layer the neighbour list of the taped positions is searched again (idmap, images, pairs)
    "large": {"lf_layer_bwd_kernel": 3, "lg_bwd_offsets_kernel": 3, "lg_colfinal_kernel": 3, "lg_colsum_kernel": 3,
              "lg_idmap_kernel": 3, "lg_images_kernel": 3, "lg_pairs_kernel": 3, "nll_bwd_kernel": 1,
              "outer_acc_kernel": 4, "outer_x3_kernel": 3, "reduce_part_kernel": 4},
    # the backward records its one-layer tape first (el_layer_tape_kernel)
    "list": {"el_bwd_offsets_kernel": 1, "el_colsum_kernel": 1, "el_layer_tape_kernel": 1,
             "lf_layer_bwd_kernel_list": 1, "outer_acc_kernel": 1, "outer_x3_kernel": 1, "reduce_part_kernel": 1},
}
CASES = list(COUNTS)


def _flow(sizes, n_layers, seed):
    """One training step's closure: (leaves, parameters) after loss.backward()."""
    from enflow_amd.data import Data
    from enflow_amd.data.synthetic import default_dt, make_molecules
    from enflow_amd.flow import Alchemical_NLL, LFIntegrator
    from enflow_amd.nn import ArgMax, EGCL
    b = make_molecules(len(sizes), sizes, nf=5, seed=seed, chain=True)
    torch.manual_seed(seed)
    model = LFIntegrator([EGCL(5, 5, 32) for _ in range(n_layers)], ArgMax(5, 32), dt=default_dt()).to(DEV)
    noise = torch.randn((int(sum(sizes)), 5), device=DEV, generator=torch.Generator(DEV).manual_seed(seed + 1))
    nll = Alchemical_NLL(kBT=1.0, softening=0.1)
    t = lambda k: torch.tensor(b[k], dtype=torch.float32, device=DEV)   # noqa: E731

    def forward():
        model.zero_grad(set_to_none=True)
        leaves = {k: t(k).requires_grad_(True) for k in ("g", "pos", "vel")}
        data = Data(h=t("h"), g=leaves["g"], pos=leaves["pos"], vel=leaves["vel"],
                    N=torch.tensor(np.diff(b["mol_ptr"])), r_cut=t("r_cut"), box=t("box"), device=DEV)
        out, ldj = model(data, noise=noise)
        loss = nll(out, ldj)
        return loss, leaves, dict(model.named_parameters())
    return forward


def _list(seed):
    from enflow_amd.nn import EGCL
    torch.manual_seed(seed)
    net = EGCL(5, 5, 32).to(DEV)
    rng = np.random.RandomState(seed)
    n, E = 40, 200                                  # two row blocks of the CSR
    row, col = rng.randint(0, n, E), rng.randint(0, n, E)
    cd, h = rand_cd(rng, E), rng.uniform(-1.0, 1.0, (n, 5)).astype(np.float32)
    w = [torch.tensor(x, device=DEV) for x in rand_weights(n, 5)]

    def forward():
        net.zero_grad(set_to_none=True)
        leaves = dict(h=torch.tensor(h, device=DEV).requires_grad_(True),
                      coord_diff=torch.tensor(cd, device=DEV).requires_grad_(True))
        lst = List(torch.tensor(row, device=DEV), torch.tensor(col, device=DEV), leaves["coord_diff"])
        loss = weighted(net.forward_edges(leaves["h"], lst), w)
        return loss, leaves, dict(net.named_parameters())
    return forward


def _case(case):
    if case == "list":
        return _list(5)
    return _flow([65, 3], 3, 4) if case == "large" else _flow([3, 22, 33], 5, 3)


def _backward(forward, timed):
    """One forward + backward: ({name: gradient}, {kernel: launches of the backward})."""
    from enflow_amd import _lib
    loss, leaves, params = forward()
    counts = {}
    if timed:
        torch.cuda.synchronize()
        with _lib.KernelTimer() as tm:
            loss.backward()
        counts = {k: n for k, (_, n) in tm.stats.items()}
    else:
        loss.backward()
    torch.cuda.synchronize()
    grads = {f"in.{k}": v.grad for k, v in leaves.items()}
    grads.update({k: p.grad for k, p in params.items()})
    missing = [k for k, g in grads.items() if g is None]
    assert not missing, f"no gradient for {missing}"
    return {k: g.clone() for k, g in grads.items()}, counts


@pytest.mark.parametrize("case", CASES)
def test_default_run_equals_the_serial_run_bitwise_and_launch_counts_hold(case, monkeypatch):
    monkeypatch.delenv("ENFLOW_SERIAL_BWD", raising=False)
    monkeypatch.delenv("ENFLOW_BWD_MIN_WS", raising=False)
    if case == "fused_min_ws":
        monkeypatch.setenv("ENFLOW_BWD_MIN_WS", "1")
    forward = _case(case)
    got, counts = _backward(forward, timed=True)
    monkeypatch.setenv("ENFLOW_SERIAL_BWD", "1")
    serial, _ = _backward(forward, timed=False)
    print(f"{case}: launches of one backward {dict(sorted(counts.items()))}")
    assert got.keys() == serial.keys()
    for k in got:
        assert torch.isfinite(got[k]).all(), k
        assert torch.equal(got[k].view(torch.int32), serial[k].view(torch.int32)), f"{case}: {k} differs"
    assert any(bool(g.any()) for k, g in got.items() if not k.startswith("in."))
    assert counts == COUNTS[case]
