"""hidden_nf 129..256 on the GPU (csrc/enflow_wide.hip) at the batch layouts
where tile code breaks, past 256 atoms per molecule and at the node_nf bounds
of the two libraries: LFIntegrator forward / reverse, EGCL and ArgMax alone,
against the float64 oracle on the same float32-rounded inputs.

The comparison is tests/test_gpu_wide_hidden.py's _check_flow: every output
tensor and log|detJ| <= 1e-5 normwise after the oracle's own float32
evaluation was asserted at half that bar, the reverse of the GPU's output
against the oracle, dequantised h exact, and zero fp32 re-runs (the f16x3
kernel itself produced the f16x3 result).  Every flow case runs at f16x3 and
f32; each asserts, on the CPU and before the GPU call, the layout it is there
for (edge count, multiplicity, the atom without an edge, max_n > 256, the
library that serves its node_nf).  Every flow case also holds Q, F and G of
its first layer alone to the bar (_check_first_layer: the flow's tensors
cannot see the forces at the reference's initialisation).

The forward reference of a case (float64 oracle and its float32 floor) is
computed once and shared by the case's precisions and row-block sizes.
"""
import functools

import numpy as np
import pytest
import torch

from _fixtures import normwise, scalar_rel, assert_all_within
from _wide import cast, f32, oracle_params
from oracle import enflow_oracle as O
import test_gpu_wide_hidden as WH
from test_gpu_wide_hidden import _check_flow, _model, _refs, _rev_ref, _rev_ldj_ref, _data  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = WH.TOL
KEYS = WH.KEYS


def _one_hot(b, seed):
    n, nf = b["h"].shape
    b["h"] = np.eye(nf)[np.random.default_rng(seed).integers(0, nf, n)]
    return b


def _mol(*a, **kw):
    from enflow_amd.data.synthetic import make_molecules
    return f32(make_molecules(*a, **kw))


def _lj(*a, **kw):
    from enflow_amd.data.synthetic import make_lj_systems
    return f32(make_lj_systems(*a, **kw))


VARIANT = dict(attention=True, norm_diff=True, tanh=True)
# id -> (model arguments of _model(hid, nf, kind, seed, n_layers, **kw), batch, noise seed, forced rows)
CASES = {
    # a 1-atom molecule (a row block without a pair), a 2-atom one, fewer atoms than a tile has pairs
    "tiny": ((256, 5, "argmax", 101), lambda: _mol(4, [1, 2, 22, 5], nf=5, seed=7), 1, (None, 32)),
    # no pair in the batch: every block skips the pair loop
    "nopairs": ((256, 5, "argmax", 102), lambda: _mol(4, [1, 1, 2, 3], nf=5, seed=22, r_cut_ang=0.5), 2, (None, 32)),
    # periodic multiplicities above 1 (a 5 A box at a 3 A cut-off)
    "mult": ((256, 5, "argmax", 103), lambda: _mol(4, [22, 31, 9, 2], nf=5, seed=7, r_cut_ang=3.0, box_ang=5.0), 3,
             (None,)),
    # rows without a pair inside blocks that have some (tests/test_gpu_grad_edges.py: seed 14 has one)
    "sparse": ((256, 5, "argmax", 104), lambda: _mol(5, [22, 31, 9, 17, 2], nf=5, seed=14, r_cut_ang=1.6), 4, (None,)),
    # molecules of rbl + 1, 2 rbl and rbl atoms at 32 rows per block; padded width, Floor
    "blocks": ((160, 5, "floor", 105), lambda: _one_hot(_mol(3, [33, 64, 32], nf=5, seed=9, radius=5.7), 1), 5,
               (None, 8, 16, 32)),
    # a molecule past 256 atoms: max_n stride, column labels past 8 bits, 75 (auto) / 10 (32 rows) blocks
    "lj300": ((256, 5, "argmax", 106), lambda: _lj([300, 5], nf=5, seed=3), 6, (None, 32)),
    "lj260var": ((256, 5, "argmax", 107, 2, VARIANT), lambda: _lj([260], nf=5, seed=4), 7, (None,)),
    # eight layers: ldj_blk accumulates per layer, h2 / pos2 ping-pong four times
    "L8": ((256, 5, "argmax", 120, 8), lambda: _mol(2, [22, 9], nf=5, seed=30), 8, (None,)),
    # both ends of the padded range
    "h129": ((129, 5, "argmax", 121), lambda: _mol(2, [22, 9], nf=5, seed=31), 9, (None,)),
    "h255": ((255, 5, "floor", 122), lambda: _one_hot(_mol(2, [22, 9], nf=5, seed=32), 2), 10, (None,)),
}
# node_nf at the library bounds: 1 and 8 on the 8-feature library, 9 and 16 on the 16-feature one
LIB_OF_NF = {1: 8, 8: 8, 9: 16, 16: 16}
for _nf in LIB_OF_NF:
    CASES[f"nf{_nf}"] = ((256, _nf, "argmax", 110 + _nf),
                         functools.partial(_mol, 3, [9, 22, 13], nf=_nf, seed=20 + _nf), 10 + _nf, (None,))

FLOW_PARAMS = [pytest.param(c, r, p, id=f"{c}-rows{r or 'auto'}-{p}")
               for c, v in CASES.items() for r in v[3] for p in ("f16x3", "f32")]


@functools.lru_cache(maxsize=None)
def _batch(case):
    """The case's float32-rounded batch, after asserting its layout premise on the CPU."""
    b = CASES[case][1]()
    _premise(case, b)
    return b


def _premise(case, b):
    """The layer-0 neighbour list has the property the case is named for."""
    from enflow_amd import _lib
    ptr = b["mol_ptr"]
    n, sizes = int(ptr[-1]), np.diff(ptr)
    row, col, _ = O.batch_edges(b["pos"], b["box"], b["r_cut"], ptr)
    if case == "tiny":
        assert len(row) == 472 and ptr[1] == 1 and 0 not in row and 0 not in col
    elif case == "nopairs":
        assert len(row) == 0
    elif case == "mult":
        assert int(O.pair_multiplicity(row, col, n)[2].max()) >= 2
    elif case == "sparse":
        lone = set(range(n)) - set(row.tolist())
        mol_of = np.searchsorted(ptr, sorted(lone), side="right") - 1
        assert len(lone) >= 1 and (sizes[mol_of] > 1).any()
    elif case == "blocks":
        assert sizes.tolist() == [32 + 1, 2 * 32, 32]
    elif case == "lj300":
        assert int(sizes.max()) > 256 and len(row) == 17708
    elif case == "lj260var":
        assert int(sizes.max()) > 256
    elif case.startswith("nf"):
        nf = b["h"].shape[1]
        assert _lib.lib(nf).enflow_max_node_nf() == LIB_OF_NF[nf]
    if case not in ("nopairs",):
        assert len(row) > 0


def _case_model(case):
    args = CASES[case][0]
    kw = args[5] if len(args) > 5 else {}
    model = _model(*args[:5], **kw)
    if case in ("h129", "h255") or case.startswith("nf"):
        assert all(n.wide and n.kernel_hidden == 256 for n in model.networks)
    return model


_FWD_REFS = {}


def _shared_refs(case):
    """_refs of the case, evaluated once: (float64 state, log|detJ|) with its float32 floor asserted."""
    def refs(model, b, noise, kind):
        if case not in _FWD_REFS:
            _FWD_REFS[case] = (None if noise is None else noise.copy(), _refs(model, b, noise, kind))
        nz, ref = _FWD_REFS[case]
        assert np.array_equal(nz, noise)       # the same draw, so the same reference
        return {k: v.copy() for k, v in ref[0].items()}, ref[1]
    return refs


def _force_rows(monkeypatch, rows):
    """Rows per block of the large-system kernels (None: the host's choice, 4 at these sizes)."""
    if rows is not None:
        monkeypatch.setenv("ENFLOW_LARGE_ROWS", str(rows))


# 1. the flow at every layout, both precisions, forced row blocks
@pytest.mark.parametrize("case,rows,prec", FLOW_PARAMS)
def test_flow_layouts(case, rows, prec, monkeypatch):
    _force_rows(monkeypatch, rows)
    monkeypatch.setattr(WH, "_refs", _shared_refs(case))
    b = _batch(case)
    kind = CASES[case][0][2]
    model = _case_model(case)
    _check_first_layer(case, model, b)
    print(case, end=" ")
    _check_flow(model, b, kind, CASES[case][2], prec)


_LAYER_REFS = {}


def _check_first_layer(case, model, b):
    """Q, F, G of the flow's first layer alone on the case's batch, each at the bar.  The flow's
    own comparisons cannot see the forces: at the reference's initialisation (coord_nn.2: xavier
    gain 0.001) |F| dt is 1e-9 .. 2e-8 of |vel| on these batches, below float32's resolution of
    vel, and |G| dt is 1e-3 .. 2e-2 of |g|; a force sum without its multiplicities passes them."""
    net = model.networks[0]
    if case not in _LAYER_REFS:
        _LAYER_REFS[case] = _egcl_refs(net, b)
    ref = _LAYER_REFS[case]
    d = _data(b)
    with torch.no_grad():
        out = [t.cpu().numpy() for t in net(d.h, d.edges)]
    e = {}
    for k, a, r in zip("QFG", out, ref):
        assert a.shape == r.shape
        if r.any():
            e[k] = normwise(a, r)
        else:               # no pair anywhere: exactly zero
            assert k == "F" and not a.any()
    print(f"{case} first layer alone:", {k: f"{v:.2e}" for k, v in e.items()})
    assert_all_within(e, TOL, "first layer alone")


# 2. per-molecule log|detJ| in both directions; 1-atom molecules on their own
@pytest.mark.parametrize("case,rows", [("tiny", None), ("tiny", 32), ("nopairs", None), ("lj300", None), ("lj300", 32)],
                         ids=lambda v: f"rows{v or 'auto'}" if not isinstance(v, str) else v)
def test_per_molecule_ldj(case, rows, monkeypatch):
    _force_rows(monkeypatch, rows)
    b = _batch(case)
    M = len(b["mol_ptr"]) - 1
    model = _case_model(case)
    d = _data(b)
    noise = torch.randn(d.h.shape, device=DEV, generator=torch.Generator(DEV).manual_seed(CASES[case][2]))
    with torch.no_grad():
        out, ldj = model(_data(b), noise=noise)
        out2, ldj_mol = model(_data(b), noise=noise, per_molecule=True)
    assert ldj_mol.shape == (M,)
    assert abs(float(ldj_mol.double().sum()) - float(ldj)) <= 1e-6 * max(abs(float(ldj)), 1.0)
    for k in KEYS:
        assert torch.equal(getattr(out, k), getattr(out2, k)), k
    want = _rev_ldj_ref(model, b, out)
    with torch.no_grad():
        _, rev = model.reverse(out.clone(), return_ldj=True)
    rev = rev.cpu().numpy()
    assert rev.shape == (M,)
    e = normwise(rev, want[np.float64])
    print(f"{case} reverse per-molecule log|detJ|: {e:.2e}")
    assert e <= TOL
    # a normwise bar over the vector would hide a 1-atom molecule behind the 22-atom one
    for m in np.flatnonzero(np.diff(b["mol_ptr"]) == 1):
        assert scalar_rel(want[np.float32][m], want[np.float64][m]) <= TOL / 2
        e1 = scalar_rel(rev[m], want[np.float64][m])
        print(f"  molecule {m} (1 atom): {e1:.2e}")
        assert e1 <= TOL


def _egcl_refs(net, b, cw=1.0):
    """float64 oracle (Q, F, G) of EGCL alone after asserting its float32 evaluation at half the bar
    (an all-zero tensor of the float64 oracle must be all zero in float32 too)."""
    ref = {}
    for dt in (np.float64, np.float32):
        c = cast(b, dt)
        ref[dt] = O._layer(oracle_params(net, dt), c["h"], c["pos"], c["box"], c["r_cut"], c["mol_ptr"], dt(cw))
    e32 = {k: normwise(a, r) if r.any() else float(np.abs(a).max(initial=0.0))
           for k, a, r in zip("QFG", ref[np.float32], ref[np.float64])}
    assert_all_within(e32, TOL / 2, "float32 CPU evaluation of EGCL")
    return ref[np.float64]


# 3. exact zeros: forces of atoms without a pair
@pytest.mark.parametrize("case", ["nopairs", "tiny"])
def test_force_of_an_atom_without_pairs_is_exactly_zero(case):
    from enflow_amd.nn import EGCL
    b = _batch(case)
    torch.manual_seed(130)
    net = EGCL(5, 5, 256).to(DEV)
    rq, rf, rg = _egcl_refs(net, b)
    d = _data(b)
    with torch.no_grad():
        q, f, g = net(d.h, d.edges)
    q, f, g = (t.cpu().numpy() for t in (q, f, g))
    e = {"Q": normwise(q, rq), "G": normwise(g, rg)}
    if case == "nopairs":
        assert not rf.any() and f.shape == rf.shape and not f.any()
    else:
        assert not rf[0].any() and not f[0].any()
        e["F"] = normwise(f, rf)
    print(f"EGCL alone on {case}:", {k: f"{v:.2e}" for k, v in e.items()})
    assert_all_within(e, TOL, f"EGCL(5, 5, 256) on {case}")


# 4. bitwise reproducible past 256 atoms (75 row blocks per molecule)
def test_bitwise_reproducible_lj300():
    b = _batch("lj300")
    model = _case_model("lj300")
    noise = torch.randn(b["h"].shape, device=DEV, generator=torch.Generator(DEV).manual_seed(6))
    with torch.no_grad():
        o1, l1 = model(_data(b), noise=noise)
        o2, l2 = model(_data(b), noise=noise)
        r1, j1 = model.reverse(o1.clone(), return_ldj=True)
        r2, j2 = model.reverse(o2.clone(), return_ldj=True)
    assert torch.equal(l1, l2) and torch.equal(j1, j2)
    for k in KEYS:
        assert torch.equal(getattr(o1, k), getattr(o2, k)), k
        assert torch.equal(getattr(r1, k), getattr(r2, k)), k


# 5. the modules alone
@pytest.mark.parametrize("fin,fout", [(3, 5), (6, 2), (1, 8)])
def test_egcl_input_output_widths(fin, fout):
    """EGCL(input_nf != output_nf, 256): run at the kernel width max(in, out) with zero-padded
    features (tests/test_gpu_shapes.py::test_egcl_input_output_widths at width 256)."""
    from enflow_amd.nn import EGCL
    b = _mol(3, [22, 40, 9], nf=fin, seed=88)
    b["h"] = np.random.default_rng(8).normal(size=b["h"].shape).astype(np.float32).astype(np.float64)
    torch.manual_seed(88)
    net = EGCL(fin, fout, 256).to(DEV)
    ref = _egcl_refs(net, b)
    d = _data(b)
    with torch.no_grad():
        out = net(d.h, d.edges)
    assert out[2].shape == (71, fout)
    e = {k: normwise(a.cpu().numpy(), r) for k, a, r in zip("QFG", out, ref)}
    print(f"EGCL({fin}, {fout}, 256):", {k: f"{v:.2e}" for k, v in e.items()})
    assert_all_within(e, TOL, f"EGCL({fin}, {fout}, 256)")


def test_egcl_coords_weight_past_256_atoms():
    """coords_weight 0.5 with every constructor variant on the 260-atom box (mode 2 stores at a
    max_n stride above 256): F scales with the weight, Q and G do not see it."""
    from enflow_amd.nn import EGCL
    b = _batch("lj260var")
    torch.manual_seed(131)
    net = EGCL(5, 5, 256, coords_weight=0.5, **VARIANT).to(DEV)
    ref = _egcl_refs(net, b, 0.5)
    d = _data(b)
    with torch.no_grad():
        out = net(d.h, d.edges)
        net.coords_weight = 1.0
        one = net(d.h, d.edges)
    e = {k: normwise(a.cpu().numpy(), r) for k, a, r in zip("QFG", out, ref)}
    print("EGCL(coords_weight=0.5) on 260 atoms:", {k: f"{v:.2e}" for k, v in e.items()})
    assert_all_within(e, TOL, "EGCL(5, 5, 256, coords_weight=0.5)")
    assert torch.equal(out[0], one[0]) and torch.equal(out[2], one[2])
    assert normwise(out[1].cpu().numpy(), 0.5 * one[1].cpu().double().numpy()) <= 1e-6


@pytest.mark.parametrize("n", [1, 32, 33, 64])
@pytest.mark.parametrize("nf", [16, 5])
def test_argmax_alone(nf, n):
    """wide_argmax_kernel works in blocks of 32 atoms: one atom, a full block, a 1-atom tail, two full blocks."""
    from enflow_amd.nn import ArgMax
    torch.manual_seed(140 + nf)
    am = ArgMax(nf, 256).to(DEV)
    hq = np.eye(nf)[np.random.default_rng(n).integers(0, nf, size=n)]
    eps = torch.randn((n, nf), device=DEV, generator=torch.Generator(DEV).manual_seed(n))
    z64, lq64 = O.argmax_forward(oracle_params(am), hq, eps.cpu().double().numpy())
    z32, lq32 = O.argmax_forward(oracle_params(am, np.float32), hq.astype(np.float32), eps.cpu().numpy())
    assert normwise(z32, z64) <= TOL / 2 and scalar_rel(lq32, lq64) <= TOL / 2
    with torch.no_grad():
        z, lq = am(torch.tensor(hq, dtype=torch.float32, device=DEV), noise=eps)
    e = {"z": normwise(z.cpu().numpy(), z64), "log_q": scalar_rel(float(lq), lq64)}
    print(f"ArgMax({nf}, 256) on {n} atoms:", {k: f"{v:.2e}" for k, v in e.items()})
    assert_all_within(e, TOL, f"ArgMax({nf}, 256)")
