"""CPU checks behind LFIntegrator.reverse_grad: the float64 restatement of the
reverse (tests/_reverse_grad.py) against the numpy oracle, the hand-written
per-layer adjoint recurrence the HIP backward implements against full autograd
of that restatement, and the argument validation of the new workspace-size
entry (enflow_lf_reverse_backward_workspace_size).

Reference: enflow/flow/dynamics.py:25-37.
"""
import os

import numpy as np
import pytest
import torch

from oracle import enflow_oracle as O
from _fixtures import load, layer_params, state, n_layers, normwise, assert_all_within
import _reverse_grad as RG


@pytest.mark.parametrize("name", ["lf_h32_L3", "lf_var_h64_L3"])
def test_restatement_matches_the_numpy_oracle(name):
    """Values of the torch restatement vs oracle.enflow_oracle.lf_reverse (1e-12),
    and its per-molecule rev_ldj vs minus the oracle's Q summed per molecule."""
    inp, _ = load(name)
    layers = [layer_params(inp, i) for i in range(n_layers(inp))]
    s = state(inp)
    dt = float(inp["dt"])
    with torch.no_grad():
        out, _, _ = RG.restate(layers, s, dt)
    ref = O.lf_reverse(layers, s, dt, dequant_kind="none")
    errs = {k: normwise(out[k].numpy(), ref[k]) for k in RG.KEYS}
    # the oracle's own loop once more for Q (lf_reverse does not return it)
    t = {k: np.array(v, copy=True) for k, v in s.items()}
    M = len(s["mol_ptr"]) - 1
    ldj = np.zeros(M)
    for p in reversed(layers):
        t["h"] = t["h"] - t["g"] * dt
        t["pos"] = O.apply_pbc(t["pos"] - t["vel"] * dt, t["box"])
        q, f, g = O._layer(p, t["h"], t["pos"], t["box"], t["r_cut"], t["mol_ptr"], 1.0)
        t["g"] = t["g"] - g * dt
        t["vel"] = (t["vel"] - f * dt) / np.exp(q)
        ldj -= np.add.reduceat(q.reshape(-1), s["mol_ptr"][:-1])
    errs["ldj"] = normwise(out["ldj"].numpy(), ldj)
    print(name, errs)
    assert_all_within(errs, 1e-12, "restatement vs numpy oracle")


def _random_case(seed=5):
    from enflow_amd.nn import EGCL
    from enflow_amd.flow import LFIntegrator
    from enflow_amd.data.synthetic import make_molecules, default_dt
    b = make_molecules(3, [5, 9, 22], nf=5, seed=seed)
    torch.manual_seed(seed + 1)
    model = LFIntegrator([EGCL(5, 5, 32), EGCL(5, 5, 32, attention=True, tanh=True)], None, dt=default_dt())
    return RG.model_layers(model), b, float(model.dt)


def test_recurrence_matches_autograd():
    """The per-layer adjoint recurrence (EGCL vjp from autograd, everything else
    written out) vs autograd over the whole restatement: 2 layers, molecules of
    5, 9 and 22 atoms, every input and parameter gradient at 1e-10 normwise."""
    layers, b, dt = _random_case()
    A, M = b["h"].shape[0], len(b["mol_ptr"]) - 1
    w = RG.weights(dict(h=(A, 5), g=(A, 5), pos=(A, 3), vel=(A, 3), ldj=(M,)), seed=7)
    _, gl, gi = RG.reference(layers, b, dt, w)
    ml, mi = RG.recurrence(layers, b, dt, w)
    errs = {f"in.{k}": normwise(mi[k], gi[k]) for k in RG.KEYS}
    for i, (a, r) in enumerate(zip(ml, gl)):
        errs.update({f"p{i}.{k}": normwise(a[k], r[k]) for k in r})
    print("recurrence vs autograd:", max(errs.values()))
    assert all(np.linalg.norm(v) > 0 for v in gi.values())
    assert_all_within(errs, 1e-10, "recurrence vs autograd")


def test_workspace_size_validates_and_is_monotone():
    from enflow_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libenflow_hip.so is not built")
    L = _lib.lib()
    ws = L.enflow_lf_reverse_backward_workspace_size
    good = (3, 36, 22, 5, 32, 1024)
    assert ws(*good) > 0
    for i in (0, 1, 2, 5):                      # a negative count
        bad = list(good)
        bad[i] = -1
        assert ws(*bad) == -1
    assert ws(3, 36, 22, 0, 32, 1024) == -1     # node_nf outside 1 .. the library's width
    assert ws(3, 36, 22, L.enflow_max_node_nf() + 1, 32, 1024) == -1
    assert ws(3, 36, 22, 5, 33, 1024) == -1     # a hidden width no kernel is built for
    assert ws(3, 36, 1 << 22, 5, 32, 1024) == -1
    assert ws(3, 36, 22, 5, 32, 1 << 31) == -1  # pair_row_bound past 2^31 - 1
    assert ws(0, 0, 0, 5, 32, 0) >= 0           # an empty batch is a valid size
    for max_n in (22, 70):                      # the fused and the large-system branch
        base = ws(3, 100, max_n, 5, 32, 4096)
        assert base > 0
        assert ws(4, 100, max_n, 5, 32, 4096) >= base
        assert ws(3, 200, max_n, 5, 32, 4096) > base
        assert ws(3, 100, max_n, 5, 32, 8192) > base
        assert ws(3, 100, max_n, 5, 64, 4096) > base
    # the call itself refuses what the size refuses, and a short workspace, before touching anything
    fn = L.enflow_lf_reverse_backward_f32
    args = [3, 36, 22, 5, 32] + [None] * 9 + [2, 0, _lib.PREC_F16X3, 0.1, 1.0] + [None] * 7 + [0, 1024, None, None]
    assert fn(*args) == -1                      # NULL pointers
    args[0] = -1
    assert fn(*args) == -1
