"""The prepared edge list (enflow_amd.data.EdgeList) on the device: the HIP build of
the CSR / CSC (enflow_graph.hip) against the torch plumbing it replaces
(EGCL._list_csr / _list_csc, pinned to numpy by tests/test_edge_list_handle_host.py),
and EGCL.forward / forward_edges on the handle against the same calls on the plain
list.  Every comparison is bitwise: the build is integer work, and the arrays it
hands to the unchanged kernels are the integers torch's stable sort produces."""
import numpy as np
import pytest
import torch

from _fixtures import load, data_from_fixture, egcl_from_fixture
from _edge_list_grad import GRAPHS, List, case_inputs, rand_cd, rand_weights, weighted
from test_edge_list_handle_host import SORT_TILE
from enflow_amd import _lib
from enflow_amd.data import EdgeList
from enflow_amd.nn import EGCL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B = SORT_TILE     # edges one workgroup of the sort ranks per pass: 4 waves x 8 rounds x 64 lanes = 2048


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert _lib.lib().enflow_graph_sort_tile() == B


def dev(a, dtype=None):
    t = torch.as_tensor(np.asarray(a), device=DEV)
    return t if dtype is None else t.to(dtype)


def bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int64)


def same(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


# ---------------------------------------------------------------------------
# 1. exactness of the build
# ---------------------------------------------------------------------------
def build_cases():
    """name -> (n, row, col, index dtype)."""
    out = {}
    for kind in GRAPHS:
        n, row, col, _, _ = case_inputs(kind, 5)
        out[kind] = (n, row, col, torch.int64)
    rng = np.random.RandomState(21)
    row = np.sort(rng.randint(0, 50, 700))
    out["sorted"] = (50, row, rng.randint(0, 50, 700), torch.int64)
    out["reverse_sorted"] = (50, row[::-1].copy(), rng.randint(0, 50, 700), torch.int32)
    out["one_row_3000_of_70"] = (70, np.full(3000, 41), rng.randint(0, 70, 3000), torch.int64)
    out["n300_keys_past_8_bits"] = (300, rng.randint(0, 300, 5000), rng.randint(0, 300, 5000), torch.int64)
    out["n70000_keys_past_16_bits"] = (70000, rng.randint(0, 70000, 4097), rng.randint(0, 70000, 4097), torch.int32)
    for E in (B - 1, B, B + 1, 2 * B + 1):
        out[f"tile_edge_{E}"] = (300, rng.randint(0, 300, E), rng.randint(0, 300, E), torch.int64)
    return out


BUILD = build_cases()


@pytest.mark.parametrize("name", list(BUILD))
def test_build_equals_the_torch_plumbing(name):
    n, row, col, itype = BUILD[name]
    E = row.size
    rng = np.random.RandomState(5)
    cd64 = rng.uniform(-2, 2, (E, 3))                      # fp64 values that round when cast
    r, c = dev(row, itype), dev(col, itype)
    cd = dev(cd64, torch.float64)
    el = EdgeList(r, c, cd, num_nodes=n)
    assert el.row is r and el.col is c and el.coord_diff is cd and (el.num_nodes, el.num_edges) == (n, E)
    topo = el.topology
    row_ptr, colp, order, bad = topo.csr()
    col_ptr, col_perm = topo.csc()
    w_ptr, w_col, w_cd, w_order, w_bad = EGCL._list_csr(n, r, c, cd)
    w_cptr, w_cperm = EGCL._list_csc(n, w_col)
    for got, want, what in ((row_ptr, w_ptr, "row_ptr"), (colp, w_col, "col"), (order, w_order, "order"),
                            (col_ptr, w_cptr, "col_ptr"), (col_perm, w_cperm, "col_perm")):
        assert got.dtype == torch.int32 and got.is_contiguous(), what
        assert np.array_equal(got.cpu().numpy(), want.cpu().numpy()), (name, what)
    assert int(bad.item()) == 0 and not bool(w_bad)
    assert same(topo.gather(cd), w_cd), "gather of fp64 coord_diff"
    cd32 = cd.to(torch.float32)
    assert same(topo.gather(cd32), cd32[w_order].contiguous()), "gather of fp32 coord_diff"
    # the scatter undoes the gather, into either dtype
    g = dev(rng.uniform(-1, 1, (E, 3)), torch.float32)
    want = torch.empty_like(g)
    want[w_order] = g
    assert same(topo.scatter(g, torch.float32), want) and same(topo.scatter(g, torch.float64), want.double())
    if name == "one_row_3000_of_70":
        assert np.array_equal(order.cpu().numpy(), np.arange(E))      # one row: the caller's order, untouched
    if name == "n70000_keys_past_16_bits":
        assert int((row_ptr[1:] == row_ptr[:-1]).sum()) > 65000       # most rows are empty


# ---------------------------------------------------------------------------
# 2. same results as the plain list
# ---------------------------------------------------------------------------
_golden = {}


def golden(name):
    """(net, h, the golden's own list) of a reference golden, computed once."""
    if name not in _golden:
        inp, _ = load(name)
        nf, hid = inp["h"].shape[1], int(inp["p0.edge_nn.2.weight"].shape[0])
        net = egcl_from_fixture(inp, 0, nf, hid).to(DEV)
        d = data_from_fixture(inp, DEV)
        ref = d.edges.reference()
        _golden[name] = (net, d.h, ref.row, ref.col, ref.coord_diff)
    return _golden[name]


def synthetic(kind, hid=32):
    n, row, col, cd, h = case_inputs(kind, 5)
    torch.manual_seed(7)
    return EGCL(5, 5, hid).to(DEV), dev(h), dev(row), dev(col), dev(cd)


def case(name):
    return golden(name) if name.startswith("egcl_") else synthetic(name)


@pytest.mark.parametrize("name", ["egcl_h32", "egcl_h128_all", "egcl_nf16_h128", "hub", "two_passes_1280_edges",
                                  "repeats_and_self_loops", "n40_no_edges", "n1_no_edges"])
def test_forward_is_bitwise_the_plain_lists(name):
    net, h, row, col, cd = case(name)
    el = EdgeList(row, col, cd, num_nodes=h.shape[0])
    with torch.no_grad():
        want = net(h, List(row, col, cd))
        got = net(h, el)
        got_fe = net.forward_edges(h, el)
    for k, a, b, w in zip("QFG", got, got_fe, want):
        assert same(a, w) and same(b, w), (name, k)


def grads(net, h, edges_of, w):
    """forward_edges + backward: (outputs, d h, d coord_diff, parameter gradients)."""
    for p in net.parameters():
        p.grad = None
    ht = h.clone().requires_grad_(True)
    lst = edges_of()
    outs = net.forward_edges(ht, lst)
    weighted(outs, w).backward()
    return ([o.detach() for o in outs], ht.grad, lst.coord_diff.grad,
            {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None})


@pytest.mark.parametrize("name", ["egcl_h128_all", "hub", "two_passes_1280_edges", "random_20", "n40_no_edges"])
def test_forward_backward_is_bitwise_the_plain_lists(name):
    net, h, row, col, cd = case(name)
    n = h.shape[0]
    cd64 = cd.double()                                      # fp64 in, fp64 gradient out, in the caller's order
    w = [dev(x) for x in rand_weights(n, net.output_nf)]
    want = grads(net, h, lambda: List(row, col, cd64.clone().requires_grad_(True)), w)
    got = grads(net, h, lambda: EdgeList(row, col, cd64.clone().requires_grad_(True), num_nodes=n), w)
    for a, b in zip(got[0], want[0]):
        assert same(a, b)
    assert same(got[1], want[1]), "d h"
    assert got[2].dtype == torch.float64 and same(got[2], want[2]), "d coord_diff"
    assert got[3].keys() == want[3].keys() and len(got[3]) >= 10
    for k in want[3]:
        assert same(got[3][k], want[3][k]), k


# ---------------------------------------------------------------------------
# 3. nothing is rebuilt
# ---------------------------------------------------------------------------
def test_one_handle_serves_every_call_without_the_torch_builders(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("the prepared path called the torch CSR / CSC builder")
    net, h, row, col, cd = synthetic("random_20")
    n = h.shape[0]
    w = [dev(x) for x in rand_weights(n, 5)]
    want = grads(net, h, lambda: List(row, col, cd.clone().requires_grad_(True)), w)
    monkeypatch.setattr(EGCL, "_list_csr", staticmethod(refuse))
    monkeypatch.setattr(EGCL, "_list_csc", staticmethod(refuse))
    with pytest.raises(AssertionError):                      # the patch bites on the plain list
        with torch.no_grad():
            net(h, List(row, col, cd))
    el = EdgeList(row, col, cd, num_nodes=n)
    topo = el.topology
    with torch.no_grad():
        q, f, g = net(h, el)
    assert same(q, want[0][0]) and same(f, want[0][1]) and same(g, want[0][2])
    got = grads(net, h, lambda: el.with_coord_diff(cd.clone().requires_grad_(True)), w)
    assert same(got[1], want[1]) and same(got[2], want[2])
    sib = el.with_coord_diff(cd * 0.5)
    assert sib.topology is topo and sib.row is row and sib.col is col and sib.coord_diff is not el.coord_diff
    with torch.no_grad():
        net(h, sib)
    # three stacked layers on the one topology, backward through all three
    torch.manual_seed(9)
    layers = [EGCL(5, 5, 32).to(DEV) for _ in range(3)]
    x = h.clone().requires_grad_(True)
    cdl = cd.clone().requires_grad_(True)
    lst = el.with_coord_diff(cdl)
    y = x
    for layer in layers:
        q, f, g = layer.forward_edges(y, lst)
        y = g + q + f.sum(1, keepdim=True)
    y.sum().backward()
    assert x.grad is not None and cdl.grad is not None and cdl.grad.shape == cd.shape
    assert all(p.grad is not None for layer in layers for p in layer.parameters())
    assert lst.topology is topo and topo.builds == 1


# ---------------------------------------------------------------------------
# 4. invalidation
# ---------------------------------------------------------------------------
def test_in_place_edit_of_row_rebuilds_at_the_next_use():
    net, h, row, col, cd = synthetic("random_20")
    n = h.shape[0]
    row = row.clone()
    el = EdgeList(row, col, cd, num_nodes=n)
    with torch.no_grad():
        before = net(h, el)
    row[:30] = (row[:30] + 7) % n
    fresh = EdgeList(row.clone(), col, cd, num_nodes=n)
    with torch.no_grad():
        got, want, plain = net(h, el), net(h, fresh), net(h, List(row, col, cd))
    assert el.topology.builds == 2
    for a, b, c, d in zip(got, want, plain, before):
        assert same(a, b) and same(a, c)
    assert not same(got[2], before[2])
    for a, b in zip(el.topology.csr()[:3], fresh.topology.csr()[:3]):
        assert torch.equal(a, b)
    w = [dev(x) for x in rand_weights(n, 5)]                 # the CSC follows the rebuilt CSR
    got = grads(net, h, lambda: el.with_coord_diff(cd.clone().requires_grad_(True)), w)
    want = grads(net, h, lambda: List(row, col, cd.clone().requires_grad_(True)), w)
    assert same(got[1], want[1]) and same(got[2], want[2])


# ---------------------------------------------------------------------------
# 5. the index guard
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("which,value,itype", [("row", -1, torch.int64), ("row", "n", torch.int32),
                                               ("col", -1, torch.int32), ("col", "n", torch.int64),
                                               ("col", 2 ** 32 + 3, torch.int64)],
                         ids=["row_-1", "row_n", "col_-1", "col_n", "col_int64_past_int32"])
def test_index_guard(which, value, itype, monkeypatch):
    net, h, row, col, cd = synthetic("random_20")
    n = h.shape[0]
    row, col = row.to(itype), col.to(itype)
    t = (row if which == "row" else col).clone()
    t[t.numel() // 2] = n if value == "n" else value
    r, c = (t, col) if which == "row" else (row, t)

    def no_sync(*a, **k):
        raise AssertionError("constructing the handle read the device")
    with monkeypatch.context() as m:                          # no .item() / .cpu() / synchronize at construction
        m.setattr(torch.Tensor, "item", no_sync)
        m.setattr(torch.Tensor, "cpu", no_sync)
        m.setattr(torch.cuda, "synchronize", no_sync)
        el = EdgeList(r, c, cd, num_nodes=n)                  # does not raise
    with torch.no_grad(), pytest.raises(IndexError):
        net(h, el)
    with pytest.raises(IndexError):
        net.forward_edges(h.clone().requires_grad_(True), el)
    with torch.no_grad():                                     # the words were reset: a clean handle runs, and is right
        got, want = net(h, EdgeList(row, col, cd, num_nodes=n)), net(h, List(row, col, cd))
    for a, b in zip(got, want):
        assert same(a, b)


# ---------------------------------------------------------------------------
# 6. determinism and streams
# ---------------------------------------------------------------------------
def test_two_builds_are_equal_and_a_side_stream_matches():
    n, row, col, itype = BUILD["n300_keys_past_8_bits"]
    r, c = dev(row, itype), dev(col, itype)
    cd = dev(rand_cd(np.random.RandomState(2), row.size))
    torch.manual_seed(3)
    net = EGCL(5, 5, 32).to(DEV)
    h = dev(np.random.RandomState(4).uniform(-1, 1, (n, 5)).astype(np.float32))
    w = [dev(x) for x in rand_weights(n, 5)]
    a, b = EdgeList(r, c, cd, num_nodes=n), EdgeList(r, c, cd, num_nodes=n)
    assert a.topology is not b.topology
    for x, y in zip(a.topology.csr() + a.topology.csc(), b.topology.csr() + b.topology.csc()):
        assert torch.equal(x, y)
    want = grads(net, h, lambda: a.with_coord_diff(cd.clone().requires_grad_(True)), w)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        el = EdgeList(r, c, cd, num_nodes=n)                  # built, used and differentiated on the side stream
        got = grads(net, h, lambda: el.with_coord_diff(cd.clone().requires_grad_(True)), w)
    side.synchronize()
    for x, y in zip(el.topology.csr() + el.topology.csc(), a.topology.csr() + a.topology.csc()):
        assert torch.equal(x, y)
    for x, y in zip(got[0], want[0]):
        assert same(x, y)
    assert same(got[1], want[1]) and same(got[2], want[2])
    for k in want[3]:
        assert same(got[3][k], want[3][k]), k


# ---------------------------------------------------------------------------
# 7. refusals unchanged
# ---------------------------------------------------------------------------
def test_refusals_are_the_plain_lists():
    net, h, row, col, cd = synthetic("random_20")
    el = EdgeList(row, col, cd, num_nodes=h.shape[0])
    with pytest.raises(NotImplementedError, match="forward_edges"):
        net(h.clone().requires_grad_(True), el)
    with pytest.raises(NotImplementedError, match="no_grad"):          # the parameters alone ask for it too
        net(h, el)
    torch.manual_seed(1)
    wide = EGCL(5, 5, 256).to(DEV)
    for call in (wide, wide.forward_edges):
        with torch.no_grad(), pytest.raises(NotImplementedError, match="up to hidden_nf 128; at hidden_nf 256"):
            call(h, el)
    with pytest.raises(ValueError, match="prepared for 20"):
        with torch.no_grad():
            net(h[:10], el)
