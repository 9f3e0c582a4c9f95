"""EGCL.forward on a caller-supplied edge list (row, col, coord_diff):
enflow_egcl_forward_list_f32 / el_layer_kernel, from the kernel up to the module.

Every comparison is normwise per tensor through _fixtures.rel_err at the
project's TOL = 1e-5: against the reference goldens' Q / F / G, against
oracle.enflow_oracle.egcl_forward on the explicit list (pinned to the reference
at 1e-12 by tests/test_oracle_golden.py), and between the list path and the
Data.edges handle path (both fp32; measured differences are printed).  The
oracle is fed what the device is fed: fp32 weights, features and coord_diff,
widened to float64."""
import numpy as np
import pytest
import torch

from oracle import enflow_oracle as O
from _fixtures import load, data_from_fixture, egcl_from_fixture, layer_params, rel_err, EGCL_KEYS
from enflow_amd import _lib
from enflow_amd.nn import EGCL

pytestmark = pytest.mark.gpu
TOL = 1e-5
DEV = "cuda:0"

GOLDENS = ["egcl_h32", "egcl_h128", "egcl_h64_att", "egcl_h32_nd_tanh", "egcl_h128_all", "egcl_act_gelu",
           "egcl_nf16_h128"]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


class List:
    """A duck-typed edge list: what the reference's EGCL.forward reads."""

    def __init__(self, row, col, coord_diff):
        self.row, self.col, self.coord_diff = row, col, coord_diff


def f64(x):
    """The fp32 value the device sees, as float64."""
    return np.asarray(x).astype(np.float32).astype(np.float64)


def params64(p):
    return {k: (f64(v) if isinstance(v, np.ndarray) else v) for k, v in p.items()}


def errs(got, want):
    return {k: rel_err(g.cpu().numpy(), w) for k, g, w in zip("QFG", got, want)}


def assert_within(e, what):
    print(f"{what}: " + ", ".join(f"{k} {v:.3e}" for k, v in e.items()))
    assert all(np.isfinite(v) and v < TOL for v in e.values()), (what, e)


_cache = {}


def golden(name):
    """The fixture, its module and batch, the two lists and the handle path's
    outputs, computed once."""
    if name in _cache:
        return _cache[name]
    inp, out = load(name)
    nf, hid = inp["h"].shape[1], int(inp["p0.edge_nn.2.weight"].shape[0])
    net = egcl_from_fixture(inp, 0, nf, hid).to(DEV)
    d = data_from_fixture(inp, DEV)
    s = {k: inp[k].astype(np.float64) for k in ("pos", "box", "r_cut")}
    row, col, ebox = O.batch_edges(s["pos"], s["box"], s["r_cut"], inp["mol_ptr"])
    cd = O.coord_diff(s["pos"], row, col, ebox).reshape(-1, 3)
    cpu_list = List(torch.tensor(row, device=DEV), torch.tensor(col, device=DEV),
                    torch.tensor(cd, dtype=torch.float64, device=DEV))        # int64, fp64
    with torch.no_grad():
        handle = net(d.h, d.edges)
    _cache[name] = dict(inp=inp, out=out, net=net, d=d, ref=d.edges.reference(), cpu=cpu_list, handle=handle)
    return _cache[name]


# ---------------------------------------------------------------------------
# 1. the reference goldens through the list
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", GOLDENS)
def test_reference_goldens_through_the_list(name):
    c = golden(name)
    want = [c["out"][k] for k in "QFG"]
    assert c["ref"].row.numel() == c["cpu"].row.numel() > 0
    for which in ("ref", "cpu"):   # Edges.reference() on the device; the oracle's list, int64 / fp64
        with torch.no_grad():
            got = c["net"](c["d"].h, c[which])
        assert got[0].shape == (want[0].shape[0], 1) and got[0].dtype == c["d"].h.dtype
        assert_within(errs(got, want), f"{name} {which} list vs golden")
        assert_within(errs(got, [t.cpu().numpy() for t in c["handle"]]), f"{name} {which} list vs Data.edges handle")


# ---------------------------------------------------------------------------
# 2. order independence and determinism
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["egcl_h32", "egcl_h128_all"])
def test_permuted_list_matches_oracle_and_is_bitwise_reproducible(name):
    c = golden(name)
    ref = c["ref"]
    g = torch.Generator().manual_seed(5)
    perm = torch.randperm(ref.row.numel(), generator=g).to(DEV)
    lst = List(ref.row[perm], ref.col[perm], ref.coord_diff[perm])
    with torch.no_grad():
        a = c["net"](c["d"].h, lst)
        b = c["net"](c["d"].h, lst)
    want = O.egcl_forward(params64(layer_params(c["inp"], 0)), f64(c["inp"]["h"]), lst.row.cpu().numpy(),
                          lst.col.cpu().numpy(), lst.coord_diff.cpu().numpy().astype(np.float64))
    assert_within(errs(a, want), f"{name} permuted list vs oracle")
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


# ---------------------------------------------------------------------------
# 3. synthetic graphs against the oracle
# ---------------------------------------------------------------------------
def cut_params(p, hid, out_nf):
    """The first `hid` hidden units and `out_nf` outputs of a fixture layer."""
    nf = p["vel_scaling_nn.0.weight"].shape[1]
    H = p["edge_nn.2.weight"].shape[0]
    rows = lambda k: p[k][:hid]                # noqa: E731
    q = dict(p)
    for k in ("edge_nn.0.weight", "edge_nn.0.bias", "edge_nn.2.bias", "node_nn.0.bias", "coord_nn.0.bias",
              "vel_scaling_nn.0.weight", "vel_scaling_nn.0.bias"):
        q[k] = rows(k)
    for k in ("edge_nn.2.weight", "coord_nn.0.weight"):
        q[k] = p[k][:hid, :hid]
    q["node_nn.0.weight"] = p["node_nn.0.weight"][:hid, :nf + hid]   # columns: h, then the messages
    q["node_nn.2.weight"] = p["node_nn.2.weight"][:out_nf, :hid]
    q["node_nn.2.bias"] = p["node_nn.2.bias"][:out_nf]
    q["coord_nn.2.weight"] = p["coord_nn.2.weight"][:, :hid]
    q["vel_scaling_nn.2.weight"] = p["vel_scaling_nn.2.weight"][:, :hid]
    assert H >= hid
    return q


def module_of(name, hid=None, out_nf=None):
    inp, _ = load(name)
    p = layer_params(inp, 0)
    nf, H = inp["h"].shape[1], int(p["edge_nn.2.weight"].shape[0])
    if hid is None and out_nf is None:
        return egcl_from_fixture(inp, 0, nf, H).to(DEV), params64(p), nf
    p = cut_params(p, hid or H, out_nf or nf)
    net = EGCL(nf, out_nf or nf, hid or H)
    net.load_state_dict({k: torch.tensor(p[k], dtype=torch.float32) for k in EGCL_KEYS})
    return net.to(DEV), params64(p), nf


def rand_cd(rng, E):
    """coord_diff entries uniform in +-[0.3, 2]."""
    return (rng.uniform(0.3, 2.0, (E, 3)) * rng.choice([-1.0, 1.0], (E, 3))).astype(np.float32)


def graph(kind, rng):
    """(n, row, col) of a synthetic graph: the smallest that reaches its code path."""
    if kind == "n1_no_edges":
        return 1, np.zeros(0, np.int64), np.zeros(0, np.int64)
    if kind == "n33_two_blocks_empty_rows":   # second block: one row, without edges; so is row 5
        row = np.repeat([r for r in range(33) if r not in (5, 32)], 3)
        return 33, row, rng.randint(0, 33, row.size)
    if kind == "row_of_200_edges":            # spans pair tiles and wave heads
        row = np.concatenate([np.repeat(np.arange(8), 2), np.full(200, 3)])
        return 8, row, rng.randint(0, 8, row.size)
    if kind == "two_passes_1280_edges":       # 32 rows x 40 > 992 pair words: row 24 straddles the passes
        row = np.repeat(np.arange(32), 40)
        return 32, row, rng.randint(0, 32, row.size)
    if kind == "columns_in_other_blocks":
        row = np.arange(70)
        return 70, row, (row + 35) % 70
    if kind == "repeats_and_self_loops":
        row = np.concatenate([np.arange(10), np.repeat(np.arange(10), 3), [4, 4]])
        col = np.concatenate([np.arange(10), np.repeat((np.arange(10) + 1) % 10, 3), [4, 4]])
        return 10, row, col
    if kind == "random_20":
        row = rng.randint(0, 20, 90)
        return 20, row, rng.randint(0, 20, 90)
    raise KeyError(kind)


# (graph, fixture whose weights are used, hidden units kept, output features kept, index dtype)
SYNTHETIC = [
    ("n1_no_edges", "egcl_h32", None, None, torch.int64),
    ("n33_two_blocks_empty_rows", "egcl_h32", None, None, torch.int32),
    ("row_of_200_edges", "egcl_h32", None, None, torch.int64),
    ("row_of_200_edges", "egcl_h128_all", None, None, torch.int32),
    ("two_passes_1280_edges", "egcl_h32", None, None, torch.int32),
    ("two_passes_1280_edges", "egcl_h64_att", None, None, torch.int64),
    ("columns_in_other_blocks", "egcl_h32", None, None, torch.int32),
    ("repeats_and_self_loops", "egcl_h32", None, None, torch.int64),
    ("random_20", "egcl_h32", None, 3, torch.int32),       # input_nf 5 -> output_nf 3
    ("random_20", "egcl_h128", 48, None, torch.int64),     # hidden_nf 48: padded to 64
    ("random_20", "egcl_nf16_h128", None, None, torch.int32),
]


@pytest.mark.parametrize("kind,name,hid,out_nf,itype", SYNTHETIC,
                         ids=[f"{s[0]}-{s[1]}" + (f"-hid{s[2]}" if s[2] else "") + (f"-out{s[3]}" if s[3] else "")
                              for s in SYNTHETIC])
def test_synthetic_graphs_vs_oracle(kind, name, hid, out_nf, itype):
    rng = np.random.RandomState(11)
    net, p, nf = module_of(name, hid, out_nf)
    n, row, col = graph(kind, rng)
    E = row.size
    if E:   # any order: the host sorts by row
        perm = rng.permutation(E)
        row, col = row[perm], col[perm]
    cd = rand_cd(rng, E)
    h = rng.uniform(-1.0, 1.0, (n, nf)).astype(np.float32)
    if kind == "repeats_and_self_loops":
        assert np.any(row == col) and np.unique(row * n + col).size < E and np.all(np.abs(cd) >= 0.3)
    if hid:
        assert net.kernel_hidden != net.hidden_nf
    t = lambda a, dt: torch.tensor(a, device=DEV).to(dt)   # noqa: E731
    q, f, g, err = net._infer_list(t(h, torch.float32), t(row, itype), t(col, itype), t(cd, torch.float32),
                                   return_err=True)
    assert err == 0
    assert q.shape == (n, 1) and f.shape == (n, 3) and g.shape == (n, out_nf or nf)
    want = O.egcl_forward(p, h.astype(np.float64), row, col, cd.astype(np.float64))
    assert_within(errs((q, f, g), want), f"{kind} / {name}")
    if E == 0:
        assert not f.any()


def test_row_ptr_that_is_no_csr_sets_the_index_bit():
    """The C entry on its own: a decreasing / overlong row_ptr is clamped into
    the list and flagged; nothing outside the arrays is touched."""
    net, _, nf = module_of("egcl_h32")
    L = _lib.lib(nf)
    n, E = 4, 6
    i32 = lambda a: torch.tensor(a, dtype=torch.int32, device=DEV)   # noqa: E731
    col = i32([0, 1, 2, 3, 0, 1])
    cd = torch.ones((E, 3), device=DEV)
    h = torch.zeros((n, nf), device=DEV)
    for ptr, bad in (([0, 2, 3, 5, 6], False), ([0, 4, 2, 5, 6], True), ([0, 2, 3, 5, 900], True),
                     ([-7, 2, 3, 5, 6], True)):
        Q, F, G = torch.empty(n, device=DEV), torch.empty((n, 3), device=DEV), torch.empty((n, nf), device=DEV)
        err = torch.zeros(1, dtype=torch.int32, device=DEV)
        rc = L.enflow_egcl_forward_list_f32(n, E, nf, 32, _lib.ptr(i32(ptr)), _lib.ptr(col), _lib.ptr(cd), _lib.ptr(h),
                                            _lib.ptr(net.packed(h.device)), 1.0, _lib.ptr(Q), _lib.ptr(F),
                                            _lib.ptr(G), _lib.ptr(err), _lib.PREC_F32, _lib.stream_ptr(h.device))
        assert rc == 0
        assert int(err.item()) == (_lib.ERR_INDEX if bad else 0), ptr
        assert bool(torch.isfinite(Q).all() and torch.isfinite(F).all() and torch.isfinite(G).all())


# ---------------------------------------------------------------------------
# 4. the f16x3 instance
# ---------------------------------------------------------------------------
def test_f16x3_instance():
    c = golden("egcl_h128")
    ref, h = c["ref"], c["d"].h
    want = [c["out"][k] for k in "QFG"]
    *got, e = c["net"]._infer_list(h, ref.row, ref.col, ref.coord_diff, prec=_lib.PREC_F16X3, return_err=True)
    names = [k for k, b in (("ERR_SMALL", _lib.ERR_SMALL), ("ERR_RANGE", _lib.ERR_RANGE)) if e & b]
    print(f"f16x3 error word: {e} ({' | '.join(names) or 'clean'})")
    assert e & ~(_lib.ERR_SMALL | _lib.ERR_RANGE) == 0
    if e == 0:   # the flow's contract for the split precision
        assert_within(errs(got, want), "egcl_h128 f16x3 list vs golden")
    *got32, e32 = c["net"]._infer_list(h, ref.row, ref.col, ref.coord_diff, prec=_lib.PREC_F32, return_err=True)
    assert e32 == 0
    assert_within(errs(got32, want), "egcl_h128 f32 list vs golden")


# ---------------------------------------------------------------------------
# 5. the index guard
# ---------------------------------------------------------------------------
def test_index_guard():
    c = golden("egcl_h32")
    ref, h, net = c["ref"], c["d"].h, c["net"]
    n, E = h.shape[0], ref.row.numel()
    want = [c["out"][k] for k in "QFG"]
    for bad in (n, -1):
        col = ref.col.clone()
        col[E // 2] = bad
        with torch.no_grad(), pytest.raises(IndexError):
            net(h, List(ref.row, col, ref.coord_diff))
        with torch.no_grad():   # the word was reset: a clean list runs, and is right
            got = net(h, ref)
        assert_within(errs(got, want), f"clean list after col == {bad}")
    row = ref.row.clone()
    row[E // 3] = n
    with torch.no_grad(), pytest.raises(IndexError):
        net(h, List(row, ref.col, ref.coord_diff))
    with torch.no_grad():
        got = net(h, ref)
    assert_within(errs(got, want), "clean list after row == n")


# ---------------------------------------------------------------------------
# 6. autograd is refused, inference is not
# ---------------------------------------------------------------------------
def test_autograd_is_refused():
    c = golden("egcl_h32")
    ref, net = c["ref"], c["net"]
    h = c["d"].h.clone().requires_grad_()
    with pytest.raises(NotImplementedError, match="no_grad"):
        net(h, ref)
    with pytest.raises(NotImplementedError, match="Data.edges"):   # the parameters alone ask for it too
        net(c["d"].h, ref)
    with torch.no_grad():
        got = net(h, ref)
    assert not any(t.requires_grad for t in got)
    assert_within(errs(got, [c["out"][k] for k in "QFG"]), "under no_grad")
