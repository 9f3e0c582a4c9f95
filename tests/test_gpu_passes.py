"""Pair buffers that take more than one pass, and row blocks of 8, 16 and 32.

Every kernel that handles a molecule larger than one LDS pair buffer streams
its pairs through the buffer in passes and keeps accumulating into the same
agg rows:

* the fused row-blocked instance lf_flow_kernel<H, 256, .., RB = 32>
  (flow_kernel.h: block_compact(.., p0 > 0), edge_tiles(.., zero_agg = false)),
  buffer Smem<H, 256, 32>::PC = 512 pairs, molecules of 65..256 atoms, inference;
* the large-system kernels lg_layer_kernel / lf_layer_bwd_kernel<.., BIG>
  (enflow_large.hip, enflow_bwd_layer.h), buffer Smem<H, 32, 32>::PC = 32 * 31
  = 992 pairs per row block of lg_rows() = 4, 8, 16 or 32 rows.

The rest of the suite gives the first only chains (<= 358 pairs per block) and
the second only batches below 4096 atoms (lg_rows() = 4, <= 250 pairs per
block): one pass, four rows.  Dense Lennard-Jones boxes reach the rest.

What was read before the first GPU run (section 0 of the issue)
---------------------------------------------------------------
The row-block size is lg_rows(num_atoms) (enflow_large.hip): it reads
ENFLOW_LARGE_ROWS with getenv at every call (4 / 8 / 16 / 32, anything else
ignored), else the largest of 32 / 16 / 8 with num_atoms / r >= 512, else 4.
Its callers: lg_args() (B.rbl of every forward / reverse / EGCL / pair-list
entry point, per call) and lg_bwd_ws() (W.nb, the backward's boff section, per
call; the workspace-size query and the backward itself both call it, so the
variable must not change between the two -- monkeypatch.setenv holds it for
the whole test).  Consumers of B.rbl: lg_setup_kernel (blk_start, rebuilt by
every entry point), lg_pairs_kernel (rows w + 4 k of the block, k < RPW = 8:
32 rows), lg_layer_kernel, lg_dequant_kernel, lg_block_words /
lg_bwd_offsets_kernel, lf_layer_bwd_kernel<BIG> (n = min(rbl, ..) <= NMAX =
32), lg_grid() = num_atoms / rbl + num_mols + 1 >= sum ceil(n_m / rbl).
enflow_edges.hip uses only lg_image_maps (no row blocks); enflow_list.hip has
its own fixed 32-row blocks and does not read lg_rows.  Host sizing:
lg_workspace() sizes ldj_blk for blocks of 4 rows whatever rbl is (the
largest block count), so _lib.large_workspace's per-device cache (grown, never
shrunk, keyed by device only) is independent of rbl; flow/_train.py allocates
the backward workspace per call from the forward's pair_rows (sum over blocks
of (tot + 31) & ~31 at the forward's rbl) and the size query.  Pair words:
22-bit label << 5 | row (< 32) | multiplicity (<= 27) << 27.  Nothing is
cached across calls with a different block size, and no bound was found that
holds only for rbl = 4.

Every case asserts its preconditions on the CPU, from the oracle's edge list
(block_pairs below): a block with more pairs than the buffer, a row whose
pairs straddle a pass boundary, and where stated a one-pass block beside them
or a block total that is an exact multiple of the buffer.

Bars: 1e-5 normwise per output tensor and on log|detJ| (bf16: 1e-3; the
dense 256-atom box at hidden 64 measures 5.0e-5 on g, a hair over the 5e-5
that tests/test_gpu_parity.py holds its 22-atom goldens to),
5e-5 normwise per gradient tensor, 1e-5 on the loss; gradients by the method of
tests/test_gpu_grad_edges.py.  Each case first asserts that the same oracle in
float32 on the CPU is within half the bar of the float64 oracle.  Two-layer
models, hidden 32 or 64, 5 node features.
"""
import collections
import copy
import functools

import numpy as np
import pytest
import torch

from oracle import enflow_oracle as O
from oracle import enflow_oracle_grad as OG
from _fixtures import normwise, scalar_rel, worst_of, assert_all_within
from test_gpu_parity import floor_reverse_check
from test_gpu_grad_edges import _gpu_batch, _gpu_grads, _compare, _assert_f32_floor, _flat
from test_gpu_ldj_mol import rev_restated, fwd_one_restated, _floor_ok, _within, _one, L2PI

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5
BF16_TOL = 1e-3
FUSED_PC = 512      # Smem<H, 256, 32>::PC
LARGE_PC = 992      # Smem<H, 32, 32>::PC = 32 * 31
FLOATS = ("h", "g", "pos", "vel", "box", "r_cut")
VAR = dict(attention=True, norm_diff=True, tanh=True)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def fmt(errs):
    return "{" + ", ".join(f"{k}: {v:.2e}" for k, v in errs.items()) + "}"


# ---------------------------------------------------------------------------
# 1. preconditions from the oracle's edge list
# ---------------------------------------------------------------------------
def block_pairs(row, col, mol_ptr, rbl, cap):
    """Row blocks of `rbl` rows per molecule (the kernels' blocking): the unique
    (row, col) pairs of each block, and whether some row of the block has pairs
    on both sides of a multiple of `cap` (the pairs of a block are ordered by
    row, so a row's range is [sum of the rows before, + its own count))."""
    A = int(mol_ptr[-1])
    key = np.unique(np.asarray(row, dtype=np.int64) * A + np.asarray(col, dtype=np.int64))
    cnt = np.bincount(key // A, minlength=A)
    tot, straddle = [], []
    for m in range(len(mol_ptr) - 1):
        a0, a1 = int(mol_ptr[m]), int(mol_ptr[m + 1])
        for r0 in range(a0, a1, rbl):
            c = cnt[r0:min(r0 + rbl, a1)]
            end = np.cumsum(c)
            start = end - c
            straddle.append(bool(np.any((start // cap + 1) * cap < end)))
            tot.append(int(end[-1]))
    return np.array(tot), np.array(straddle)


def check_passes(name, b, rbl, cap, multi=True, straddling=True, single_beside=False, exact=False):
    """The layer-0 list of batch b has what the case is there for.  straddling
    is waived only for the 65-atom all-to-all molecule: its rows of 64 pairs
    tile the 512-pair buffer exactly, so no row can straddle there."""
    row, col, _ = O.batch_edges(b["pos"], b["box"], b["r_cut"], b["mol_ptr"])
    tot, straddle = block_pairs(row, col, b["mol_ptr"], rbl, cap)
    passes = np.maximum(1, -(-tot // cap))
    print(f"{name}: rows per block {rbl}, buffer {cap}: pairs per block {tot.min()}..{tot.max()} "
          f"({len(tot)} blocks), passes {passes.min()}..{passes.max()}, blocks with a straddling row "
          f"{int(straddle.sum())}")
    if multi:
        assert tot.max() > cap, f"{name}: no block with more than {cap} pairs"
        assert straddle.any() == straddling, f"{name}: rows straddling a pass boundary: {int(straddle.sum())}"
    if single_beside:
        assert tot.min() <= cap, f"{name}: no one-pass block"
    if exact:
        full = tot[:-1]     # one molecule: every block but its last has all its rows
        assert len(full) and full.min() > cap and np.all(full % cap == 0), \
            f"{name}: full-block totals {full} are no multiple of {cap}"
    return tot


def assert_all_to_all(b):
    """One molecule in which every row has n - 1 columns of multiplicity 1."""
    n = int(b["mol_ptr"][-1])
    row, col, _ = O.batch_edges(b["pos"], b["box"], b["r_cut"], b["mol_ptr"])
    assert len(row) == n * (n - 1) and not np.any(row == col)
    r, c, mult = O.pair_multiplicity(row, col, n)
    assert len(r) == n * (n - 1) and np.all(mult == 1)
    assert np.all(np.bincount(r, minlength=n) == n - 1)


# ---------------------------------------------------------------------------
# batches and models
# ---------------------------------------------------------------------------
def _f32(b):
    out = dict(b)
    for k in FLOATS:
        out[k] = np.asarray(b[k], dtype=np.float32).astype(np.float64)
    return out


def _cast(b, dtype):
    s = {k: np.asarray(b[k], dtype=dtype) for k in FLOATS}
    s["mol_ptr"] = np.asarray(b["mol_ptr"], dtype=np.int64)
    return s


@functools.lru_cache(maxsize=None)
def _lj(sizes, r_cut=2.5, seed=7):
    """Periodic LJ boxes, float32-representable float64 arrays (cached, never modified)."""
    from enflow_amd.data.synthetic import make_lj_systems
    return _f32(make_lj_systems(list(sizes), nf=5, seed=seed, r_cut=r_cut))


@functools.lru_cache(maxsize=None)
def _cluster(n, seed=9):
    """n atoms on a jittered grid (spacing 0.9) in which every atom sees every
    other exactly once: r_cut = the largest distance + 2 (so later layers keep
    the list), a cubic box of edge L with sqrt(2) (L - e) > L + r_cut (e = the
    half extent): every edge and corner image lies outside the reference's
    ellipsoid, the first surviving image (0, 0, -L) holds all n atoms, so
    id_mapping is the identity; L - 2 e > r_cut: no periodic image hits;
    L / 4 > 2 e: the half-box minimum image leaves coord_diff alone."""
    from enflow_amd.data.synthetic import make_lj_systems
    b = make_lj_systems([n], nf=5, seed=seed)
    rng = np.random.default_rng(seed + 1)
    side = int(np.ceil(n ** (1 / 3)))
    grid = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3)[:n]
    pos = grid * 0.9 + rng.uniform(-0.1, 0.1, size=(n, 3))
    pos = pos - pos.mean(0, keepdims=True)
    e = float(np.abs(pos).max())
    dmax = float(np.sqrt(((pos[:, None] - pos[None]) ** 2).sum(-1)).max())
    rc = dmax + 2.0
    L = float(np.ceil(max((rc + np.sqrt(2.0) * (e + 1.0)) / (np.sqrt(2.0) - 1.0), 8.0 * (e + 1.0)) + 2.0))
    b["pos"], b["box"], b["r_cut"] = pos, np.full((n, 3), L), np.array([rc])
    b = _f32(b)
    assert_all_to_all(b)
    return b


def _int_h(b, seed, scale=1.0):
    """Integer features (what Floor expects), times scale; g scaled too."""
    out = dict(b)
    rng = np.random.default_rng(seed)
    out["h"] = np.floor(rng.uniform(0, 3, size=b["h"].shape)) * scale
    out["g"] = b["g"] * scale
    return _f32(out)


def _build(kind, hid, seed, var=False, scale=1.0, small=False):
    """Two layers on the CPU, weights from torch.manual_seed(seed).  small:
    layer 1's edge_nn.0 scaled by `scale` (tests/test_gpu_small.py's "edge0")."""
    from enflow_amd.nn import EGCL, ArgMax, Floor
    from enflow_amd.flow import LFIntegrator
    from enflow_amd.data.synthetic import default_dt
    torch.manual_seed(seed)
    nets = [EGCL(5, 5, hid, **(VAR if var else {})) for _ in range(2)]
    if small:
        with torch.no_grad():
            nets[1].edge_nn[0].weight.mul_(scale)
            nets[1].edge_nn[0].bias.mul_(scale)
    dq = ArgMax(5, hid) if kind == "argmax" else Floor(dequant_scale=scale)
    model = LFIntegrator(nets, dq, dt=default_dt())
    model.build_args = (kind, hid, seed, var, scale, small)
    return model


_cpu_model = functools.lru_cache(maxsize=None)(_build)   # the oracle's side, never modified


def _on_gpu(model, prec):
    """The same model built again (same seed, same weights) on the GPU."""
    m = _build(*model.build_args).to(DEV)
    m.gemm_precision = prec
    return m


def _layers(model, dtype=np.float64):
    out = []
    for n in model.networks:
        p = {k: v.detach().cpu().double().numpy().astype(dtype) for k, v in n.state_dict().items()}
        p["flags"] = (bool(n.attention), bool(n.norm_diff), bool(n.tanh))
        out.append(p)
    return out


def _dq(model, kind, dtype=np.float64):
    if kind == "floor":
        return dtype(model.dequantize.dequant_scale)
    return {k: v.detach().cpu().double().numpy().astype(dtype) for k, v in model.dequantize.state_dict().items()}


def _data(b):
    from enflow_amd.data import Data
    return Data.from_arrays(b, device=DEV)


def _noise(b, kind, seed):
    rng = np.random.default_rng(seed)
    draw = rng.normal(size=b["h"].shape) if kind == "argmax" else rng.uniform(size=b["h"].shape)
    return draw.astype(np.float32)


# ---------------------------------------------------------------------------
# flow forward + reverse against the oracle (shared by sections 2, 3 and 4)
# ---------------------------------------------------------------------------
_FLOW_REF = {}


def _flow_ref(key, model, b, kind, noise):
    """Oracle forward of b, oracle reverse of its float32-rounded output; both
    also in float32, asserted within half the bar of float64.  Cached per key."""
    if key in _FLOW_REF:
        return _FLOW_REF[key]
    dt = model.dt
    ref, ldj = O.lf_forward(_layers(model), _dq(model, kind), b, noise.astype(np.float64), dt, dequant_kind=kind)
    r32, ldj32 = O.lf_forward(_layers(model, np.float32), _dq(model, kind, np.float32), _cast(b, np.float32), noise,
                              np.float32(dt), dequant_kind=kind)
    floor = {k: normwise(r32[k], ref[k]) for k in ("h", "g", "pos", "vel")}
    floor["ldj"] = scalar_rel(ldj32, ldj)
    st = _f32({**ref, "box": b["box"], "r_cut": b["r_cut"]})
    st["mol_ptr"] = b["mol_ptr"]
    rkind = "argmax" if kind == "argmax" else "none"     # Floor: the continuous h, floored by the check
    back = O.lf_reverse(_layers(model), st, dt, dequant_kind=rkind)
    b32 = O.lf_reverse(_layers(model, np.float32), _cast(st, np.float32), np.float32(dt), dequant_kind=rkind)
    floor.update({"rev_" + k: normwise(b32[k], back[k]) for k in ("g", "pos", "vel")})
    if kind == "argmax":
        assert np.array_equal(b32["h"], back["h"])
    print(f"{key}: float32 oracle vs float64 oracle {fmt(floor)}")
    assert_all_within(floor, TOL / 2, f"{key}: float32 oracle vs float64 oracle")
    _FLOW_REF[key] = (ref, ldj, st, back, worst_of(floor))
    return _FLOW_REF[key]


def _flow_vs_oracle(key, model, b, kind, prec, seed, expect_reruns=0, twice=False):
    """Forward and reverse on the GPU against _flow_ref; returns the errors."""
    from enflow_amd import _lib
    noise = _noise(b, kind, seed)
    ref, ref_ldj, st, rback, _ = _flow_ref(key, model, b, kind, noise)
    gm = _on_gpu(model, prec)
    nz = torch.tensor(noise, device=DEV)
    n0 = _lib.FP32_RERUNS[0]
    with torch.no_grad():
        o, ldj = gm(_data(b), noise=nz)
    reruns = _lib.FP32_RERUNS[0] - n0
    errs = {k: normwise(getattr(o, k).cpu().numpy(), ref[k]) for k in ("h", "g", "pos", "vel")}
    errs["ldj"] = scalar_rel(ldj, ref_ldj)
    with torch.no_grad():
        back = gm.reverse(_data(st))
    errs.update({"rev_" + k: normwise(getattr(back, k).cpu().numpy(), rback[k]) for k in ("g", "pos", "vel")})
    print(f"{key} {prec}: fp32 re-runs of the forward {reruns}; vs oracle {fmt(errs)}")
    if kind == "argmax":
        np.testing.assert_array_equal(back.h.cpu().numpy(), rback["h"])
    elif float(model.dequantize.dequant_scale) == 1.0:
        floor_reverse_check(back.h.cpu().numpy(), rback["h"])
    assert reruns == expect_reruns, f"{key} {prec}: {reruns} fp32 re-runs, expected {expect_reruns}"
    assert_all_within(errs, BF16_TOL if prec == "bf16" else TOL, f"{key} {prec}")
    if twice:   # bitwise reproducible
        with torch.no_grad():
            o2, ldj2 = gm(_data(b), noise=nz)
            back2 = gm.reverse(_data(st))
        for k in ("h", "g", "pos", "vel"):
            assert torch.equal(getattr(o, k), getattr(o2, k)), k
            assert torch.equal(getattr(back, k), getattr(back2, k)), k
        assert float(ldj) == float(ldj2)
    return errs


# ---------------------------------------------------------------------------
# 2. the fused row-blocked instance (65..256 atoms, inference), buffer 512
# ---------------------------------------------------------------------------
# id -> (batch, dequantiser, hidden, variants, check_passes keywords)
FUSED = {
    "lj200+70": (lambda: _lj((200, 70)), "argmax", 32, False, dict(single_beside=True)),
    "lj256+3": (lambda: _lj((256, 3)), "argmax", 64, False, dict(single_beside=True)),
    "lj97_var": (lambda: _lj((97,)), "argmax", 32, True, dict(single_beside=True)),
    "lj200+70_floor": (lambda: _int_h(_lj((200, 70)), 3), "floor", 32, False, dict(single_beside=True)),
    "all65": (lambda: _cluster(65), "argmax", 32, False, dict(exact=True, straddling=False, single_beside=True)),
}
FUSED_PARAMS = [(c, p) for c in FUSED for p in (("f32", "f16x3", "bf16") if FUSED[c][1] == "argmax" and
                                                not FUSED[c][3] else ("f32", "f16x3"))]


def _fused_case(case):
    from enflow_amd import _lib
    mk, kind, hid, var, kw = FUSED[case]
    b = mk()
    sizes = np.diff(b["mol_ptr"])
    assert 64 < sizes.max() <= 256 and not _lib.is_large(int(sizes.max()))   # the fused row-blocked instance
    tot = check_passes(case, b, 32, FUSED_PC, **kw)
    if case == "all65":     # 32 x 64 = 4 x 512 in each full block, one row of 64 pairs in the last
        assert tot.tolist() == [2048, 2048, 64]
    return b, kind, _cpu_model(kind, hid, 11, var)


@pytest.mark.parametrize("case,prec", FUSED_PARAMS, ids=["-".join(p) for p in FUSED_PARAMS])
def test_fused_blocked_flow_vs_oracle(case, prec):
    b, kind, model = _fused_case(case)
    _flow_vs_oracle(("fused", case), model, b, kind, prec, 21, twice=prec == "f16x3")


def test_fused_blocked_per_molecule_ldj():
    """reverse(return_ldj=True) (the RLDJ instance) and forward(per_molecule=True)
    on the multi-pass batch, against tests/test_gpu_ldj_mol.py's restatements."""
    b, kind, model = _fused_case("lj200+70")
    M = len(b["mol_ptr"]) - 1
    fin, ref, S = rev_restated(_layers(model), b, model.dt)
    want = O.lf_reverse(_layers(model), b, model.dt, dequant_kind="none")
    for k in ("h", "g", "pos", "vel"):
        assert np.array_equal(fin[k], want[k])
    _, r32, _ = rev_restated(_layers(model, np.float32), b, np.float32(model.dt), np.float32)
    _floor_ok("fused multi-pass reverse ldj", r32, ref, S)
    noise = _noise(b, kind, 22)
    fref, fS, f32 = np.zeros(M), np.zeros(M), np.zeros(M)
    for m in range(M):
        st1, n1 = _one(b, m, noise.astype(np.float64))
        fref[m], fS[m] = fwd_one_restated(_layers(model), _dq(model, kind), st1, n1, model.dt, kind)
        _, one = O.lf_forward(_layers(model), _dq(model, kind), st1, n1, model.dt)
        assert fref[m] == one
        f32[m], _ = fwd_one_restated(_layers(model, np.float32), _dq(model, kind, np.float32), st1, n1,
                                     np.float32(model.dt), kind, np.float32)
    _floor_ok("fused multi-pass forward per molecule", f32, fref, fS)
    gm = _on_gpu(model, "f16x3")
    nz = torch.tensor(noise, device=DEV)
    with torch.no_grad():
        plain = gm.reverse(_data(b))
        out, rev = gm.reverse(_data(b), return_ldj=True)
        fplain, scalar = gm(_data(b), noise=nz)
        fout, ldj_mol = gm(_data(b), noise=nz, per_molecule=True)
    for k in ("h", "g", "pos", "vel"):
        assert torch.equal(getattr(out, k), getattr(plain, k)), k
        assert torch.equal(getattr(fout, k), getattr(fplain, k)), k
    _within("fused multi-pass rev_ldj", rev.cpu().numpy(), ref, S)
    share = -0.5 * L2PI / M
    _within("fused multi-pass forward per molecule", ldj_mol.cpu().numpy(), fref + 0.5 * L2PI + share, fS + abs(share))
    assert abs(float(ldj_mol.double().sum()) - float(scalar)) <= 1e-6 * abs(float(scalar))


# ---------------------------------------------------------------------------
# 3. the large-system kernels at 8, 16 and 32 rows per block, buffer 992
# ---------------------------------------------------------------------------
ROWS = [8, 16, 32]


def _rcut(rbl):
    return 2.5 if rbl == 8 else 3.2     # 16 rows pass 992 pairs only at the wider cut-off


@pytest.mark.parametrize("rbl", ROWS)
def test_large_edges_exact(rbl, monkeypatch):
    """Data.edges (lg_pairs_kernel: rows w + 4 k of a block, k >= 1) and
    Edges.edge_index on [300, 37]: blocks of rbl rows, a last block of 4 or 12
    and one of 5 rows."""
    monkeypatch.setenv("ENFLOW_LARGE_ROWS", str(rbl))
    b = _lj((300, 37))
    assert 300 % rbl in (4, 12) and 37 % rbl == 5
    check_passes("edges [300, 37]", b, rbl, LARGE_PC, multi=False)
    row, col, _ = O.batch_edges(b["pos"], b["box"], b["r_cut"], b["mol_ptr"])
    e = _data(b).edges
    got = collections.Counter(zip(e.row.cpu().tolist(), e.col.cpu().tolist()))
    assert got == collections.Counter(zip(row.tolist(), col.tolist()))
    idx = e.edge_index.cpu().numpy()
    assert idx.dtype == np.int64 and idx.shape == (2, len(row))
    assert np.array_equal(idx[0], row) and np.array_equal(idx[1], col)


@pytest.mark.parametrize("prec", ["f32", "f16x3"])
@pytest.mark.parametrize("rbl", ROWS)
def test_large_flow_vs_oracle(rbl, prec, monkeypatch):
    """[300, 5]: at 16 and 32 rows (r_cut 3.2) every block of the box takes
    several passes and the 5-atom molecule's block one; 8 rows (r_cut 2.5) run
    one pass with two rows per wave in lg_pairs_kernel."""
    monkeypatch.setenv("ENFLOW_LARGE_ROWS", str(rbl))
    b = _lj((300, 5), _rcut(rbl))
    check_passes(f"flow [300, 5] r_cut {_rcut(rbl)}", b, rbl, LARGE_PC, multi=rbl > 8, single_beside=True)
    _flow_vs_oracle(("large", rbl), _cpu_model("argmax", 32, 12), b, "argmax", prec, 23, twice=prec == "f16x3")


def test_large_flow_variants_rows32(monkeypatch):
    monkeypatch.setenv("ENFLOW_LARGE_ROWS", "32")
    b = _lj((300, 5), 3.2)
    check_passes("var [300, 5] r_cut 3.2", b, 32, LARGE_PC, single_beside=True)
    _flow_vs_oracle(("large-var", 32), _cpu_model("argmax", 32, 13, True), b, "argmax", "f16x3", 24)


def _egcl_oracle(net, b, dtype=np.float64):
    p = {k: v.detach().cpu().double().numpy().astype(dtype) for k, v in net.state_dict().items()}
    p["flags"] = (bool(net.attention), bool(net.norm_diff), bool(net.tanh))
    s = _cast(b, dtype)
    row, col, eb = O.batch_edges(s["pos"], s["box"], s["r_cut"], s["mol_ptr"])
    return dict(zip("qfg", O.egcl_forward(p, s["h"], row, col, O.coord_diff(s["pos"], row, col, eb))))


def _egcl_gpu(net, b):
    d = _data(b)
    with torch.no_grad():
        q, f, g = copy.deepcopy(net).to(DEV)(d.h, d.edges)
    return dict(q=q, f=f, g=g)


def _egcl_errs(name, got, ref, r32):
    floor = {k: normwise(r32[k].reshape(-1), ref[k].reshape(-1)) for k in "qfg"}
    assert_all_within(floor, TOL / 2, f"{name}: float32 oracle vs float64 oracle")
    errs = {k: normwise(got[k].cpu().numpy().reshape(-1), ref[k].reshape(-1)) for k in "qfg"}
    print(f"{name}: vs oracle {fmt(errs)}, float32-oracle floor {worst_of(floor):.2e}")
    assert_all_within(errs, TOL, name)


def test_large_egcl_forward_rows32(monkeypatch):
    """Standalone EGCL.forward (lg_layer_kernel mode 2) in passes."""
    from enflow_amd.nn import EGCL
    monkeypatch.setenv("ENFLOW_LARGE_ROWS", "32")
    b = _lj((300,), 3.2)
    check_passes("EGCL [300] r_cut 3.2", b, 32, LARGE_PC)
    torch.manual_seed(14)
    net = EGCL(5, 5, 64)
    _egcl_errs("EGCL forward, 32 rows", _egcl_gpu(net, b), _egcl_oracle(net, b), _egcl_oracle(net, b, np.float32))


@functools.lru_cache(maxsize=None)
def _train_ref(case):
    """(batch, CPU model, noise, (loss, grads) float64, float32-oracle floor)."""
    from enflow_amd.data.synthetic import default_kBT
    b = _cluster(311) if case == "all311" else _lj((300,), 3.2)
    model = _cpu_model("argmax", 64, 15)
    eps = _noise(b, "argmax", 25)
    layers = [{k: v.detach().double().numpy() for k, v in n.named_parameters()} for n in model.networks]
    dq = {k: v.detach().double().numpy() for k, v in model.dequantize.named_parameters()}
    res = []
    for dtype in (torch.float64, torch.float32):
        loss, _, gl, gd, _, gi = OG.train_loss_and_grads(layers, dq, b, eps.astype(np.float64), model.dt,
                                                         default_kBT(), 0.1, dtype=dtype, input_grads=True)
        res.append((loss, _flat(gl, gd, gi)))
    return b, model, eps, res[0], _assert_f32_floor(f"train {case}", *res)


def _train_step(gm, b, eps):
    from enflow_amd.flow import Alchemical_NLL
    from enflow_amd.data.synthetic import default_kBT
    gm.zero_grad(set_to_none=True)
    data, leaves = _gpu_batch(b)
    out, ldj = gm(data, noise=torch.tensor(eps, device=DEV))
    loss = Alchemical_NLL(kBT=default_kBT(), softening=0.1)(out, ldj)
    loss.backward()
    return float(loss.detach()), _gpu_grads(gm, leaves)


def _train_vs_oracle(name, case, prec):
    from enflow_amd import _lib
    b, model, eps, ref, floor = _train_ref(case)
    gm = _on_gpu(model, prec)
    n0 = _lib.FP32_RERUNS[0]
    loss, got = _train_step(gm, b, eps)
    assert _lib.FP32_RERUNS[0] == n0, f"{name}: the training forward was re-run in fp32"
    _compare(name, loss, got, ref, floor)
    loss2, got2 = _train_step(gm, b, eps)      # bitwise reproducible
    assert loss2 == loss
    for k in got:
        assert np.array_equal(got[k], got2[k]), k


@pytest.mark.parametrize("prec", ["f16x3", "f32"])
@pytest.mark.parametrize("rbl", [16, 32])
def test_large_training_vs_oracle(rbl, prec, monkeypatch):
    """One training step on [300] at r_cut 3.2: the tape forward, pair_rows,
    lg_bwd_offsets_kernel and lf_layer_bwd_kernel<BIG> in several passes (gt,
    Rw, tmax past the first); loss, every parameter, dequantiser and input
    gradient against the gradient oracle; a second step bitwise equal."""
    monkeypatch.setenv("ENFLOW_LARGE_ROWS", str(rbl))
    check_passes("train [300] r_cut 3.2", _train_ref("lj300")[0], rbl, LARGE_PC)
    _train_vs_oracle(f"train [300] {rbl} rows {prec}", "lj300", prec)


def test_large_egcl_backward_rows32(monkeypatch):
    """Standalone EGCL backward past 64 atoms (enflow_egcl_backward_large_f32) in passes."""
    from enflow_amd.nn import EGCL
    monkeypatch.setenv("ENFLOW_LARGE_ROWS", "32")
    b = _lj((300,), 3.2)
    check_passes("EGCL backward [300] r_cut 3.2", b, 32, LARGE_PC)
    torch.manual_seed(16)
    net = EGCL(5, 5, 64)
    rng = np.random.default_rng(26)
    w = dict(q=rng.normal(size=(300, 1)), f=rng.normal(size=(300, 3)), g=rng.normal(size=(300, 5)))
    w = {k: v.astype(np.float32) for k, v in w.items()}
    row, col, eb = O.batch_edges(b["pos"], b["box"], b["r_cut"], b["mol_ptr"])
    res = []
    for dtype in (torch.float64, torch.float32):
        t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64)).to(dtype)  # noqa: E731
        P = {k: t(v.detach().numpy()).requires_grad_(True) for k, v in net.named_parameters()}
        h, pos = t(b["h"]).requires_grad_(True), t(b["pos"]).requires_grad_(True)
        q, f, g = OG._egcl(P, h, pos, torch.as_tensor(row), torch.as_tensor(col), t(eb), 300, float(net.coords_weight))
        loss = (q * t(w["q"])).sum() + (f * t(w["f"])).sum() + (g * t(w["g"])).sum()
        loss.backward()
        grads = {k: v.grad.double().numpy() for k, v in P.items()}
        grads.update({"in.h": h.grad.double().numpy(), "in.pos": pos.grad.double().numpy()})
        res.append((float(loss.detach()), grads))
    floor = _assert_f32_floor("EGCL backward, 32 rows", *res)
    gnet = copy.deepcopy(net).to(DEV)
    d = _data(b)
    d.h.requires_grad_(True)
    d.pos.requires_grad_(True)
    q, f, g = gnet(d.h, d.edges)
    t32 = lambda a: torch.tensor(a, device=DEV)  # noqa: E731
    loss = (q * t32(w["q"])).sum() + (f * t32(w["f"])).sum() + (g * t32(w["g"])).sum()
    loss.backward()
    torch.cuda.synchronize()
    got = {k: p.grad.double().cpu().numpy() for k, p in gnet.named_parameters()}
    got.update({"in.h": d.h.grad.double().cpu().numpy(), "in.pos": d.pos.grad.double().cpu().numpy()})
    _compare("EGCL backward, 32 rows", float(loss.detach()), got, res[0], floor)


def test_large_exact_multiple_rows32(monkeypatch):
    """311 atoms that all see each other once: 32 x 310 = 10 x 992 pairs in each
    full block (the last pass of a block is a full buffer), 23 rows in the last."""
    monkeypatch.setenv("ENFLOW_LARGE_ROWS", "32")
    b = _cluster(311)
    tot = check_passes("all311", b, 32, LARGE_PC, exact=True)
    assert tot.tolist() == [9920] * 9 + [23 * 310]
    _flow_vs_oracle(("large", "all311"), _cpu_model("argmax", 32, 12), b, "argmax", "f16x3", 27)
    _train_vs_oracle("train all311 32 rows f16x3", "all311", "f16x3")


@pytest.mark.parametrize("boxes,rbl", [(14, 8), (28, 16)])
def test_large_rows_chosen_by_batch_size(boxes, rbl, monkeypatch):
    """Without the variable: 4200 atoms run 8 rows per block, 8400 atoms 16
    (lg_rows(): the largest of 32 / 16 / 8 with num_atoms / r >= 512).  A
    one-layer EGCL forward against the oracle, bitwise the forced run's."""
    from enflow_amd.nn import EGCL
    monkeypatch.delenv("ENFLOW_LARGE_ROWS", raising=False)
    b = _lj((300,) * boxes)
    A = 300 * boxes
    assert A // rbl >= 512 > A // (2 * rbl)
    torch.manual_seed(17)
    net = EGCL(5, 5, 32)
    got = _egcl_gpu(net, b)
    _egcl_errs(f"EGCL forward, {boxes} boxes", got, _egcl_oracle(net, b), _egcl_oracle(net, b, np.float32))
    monkeypatch.setenv("ENFLOW_LARGE_ROWS", str(rbl))
    forced = _egcl_gpu(net, b)
    for k in "qfg":
        assert torch.equal(got[k], forced[k]), k


# ---------------------------------------------------------------------------
# 4. the F16X3 small-operand word (sm.big) across passes
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["fused", "rows32"])
def test_small_operands_across_passes(which, monkeypatch):
    """tests/test_gpu_small.py's recipe at 1e-3 on a multi-pass batch: the f16x3
    forward flags ENFLOW_ERR_SMALL, is re-run once with fp32 GEMMs and then meets
    the bar.  (The unscaled multi-pass batches above must count no re-run: a
    word reset between passes would flag their short last passes.)"""
    scale = 1e-3
    if which == "fused":
        b = _int_h(_lj((200, 70)), 4, scale)
        check_passes("small fused", b, 32, FUSED_PC)
    else:
        monkeypatch.setenv("ENFLOW_LARGE_ROWS", "32")
        b = _int_h(_lj((300,), 3.2), 4, scale)
        check_passes("small 32 rows", b, 32, LARGE_PC)
    model = _cpu_model("floor", 64, 18, scale=scale, small=True)
    _flow_vs_oracle(("small", which), model, b, "floor", "f16x3", 28, expect_reruns=1)
