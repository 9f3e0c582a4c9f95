"""CPU-only checks of the prepared edge list (enflow_amd.data.EdgeList, enflow_graph.hip):

(a) the class is exported, is not an Edges, and is still "an object with row, col
    and coord_diff";
(b) every shape refusal is a ValueError, the kernels' limits a NotImplementedError
    with the plain list's text, CPU tensors a HipPathError -- in that order, so each
    is the same on any machine;
(c) the new C entries: declared, bound with the header's argument count, exported
    by both libraries without an ABI bump, argument errors before any launch;
(d) what the device build must return, stated in numpy (stable sort by clamped row,
    row_ptr, clamped col, CSC) and pinned to tests/_edge_list_grad.csc_numpy and to
    EGCL._list_csr / _list_csc on the CPU; tests/test_gpu_edge_list_handle.py compares
    the HIP build to the same torch functions on the device."""
import types

import numpy as np
import pytest
import torch

from _edge_list_grad import GRAPHS, csc_numpy, graph
from test_edge_list_egcl_host import header_prototypes
from enflow_amd import _lib
from enflow_amd.data import Edges, EdgeList
from enflow_amd.nn import EGCL

ENTRIES = {"enflow_graph_sort_tile": 0, "enflow_graph_workspace_size": 2, "enflow_graph_csr_build": 13,
           "enflow_graph_csc_build": 8, "enflow_graph_gather_f32": 6, "enflow_graph_scatter_f32": 6}
SORT_TILE = 2048      # edges one workgroup of the sort ranks (4 waves x 8 rounds x 64 lanes)


# ---------------------------------------------------------------------------
# (a) the class
# ---------------------------------------------------------------------------
def test_exported_and_not_an_edges_handle():
    import enflow_amd.data as data
    assert data.EdgeList is EdgeList
    assert not issubclass(EdgeList, Edges)
    for k in ("row", "col", "num_nodes", "num_edges", "with_coord_diff"):
        assert hasattr(EdgeList, k), k


def stub(n=3, E=2, cd=None):
    """A handle around a topology that was never built (no GPU here): the checks
    that come before any device work."""
    topo = types.SimpleNamespace(row=torch.tensor([0, 1][:E]), col=torch.tensor([1, 2][:E]), num_nodes=n, num_edges=E)
    el = EdgeList(None, None, None, _topology=topo)
    el.coord_diff = cd
    return el


def test_stub_carries_row_col_coord_diff_and_shares_its_topology():
    el = stub(cd=torch.zeros((2, 3)))
    assert all(hasattr(el, k) for k in ("row", "col", "coord_diff"))
    assert (el.num_nodes, el.num_edges) == (3, 2)
    assert not isinstance(el, Edges)


# ---------------------------------------------------------------------------
# (b) refusals
# ---------------------------------------------------------------------------
def test_shape_mismatches_are_value_errors():
    row, col = torch.tensor([0, 1]), torch.tensor([1, 2])
    with pytest.raises(ValueError, match="cols"):
        EdgeList(row, torch.tensor([1, 2, 0]), num_nodes=3)
    with pytest.raises(ValueError, match="coord_diff"):
        EdgeList(row, col, torch.zeros((3, 3)), num_nodes=3)
    with pytest.raises(ValueError, match="coord_diff"):
        EdgeList(row, col, torch.zeros((2, 2)), num_nodes=3)
    with pytest.raises(ValueError, match="coord_diff"):
        EdgeList(row, col, torch.zeros(6), num_nodes=3)
    with pytest.raises(ValueError, match="num_nodes"):
        EdgeList(row, col, torch.zeros((2, 3)))
    with pytest.raises(ValueError, match="int32 or int64"):
        EdgeList(row.float(), col, num_nodes=3)
    with pytest.raises(ValueError, match="coord_diff"):        # a sibling is checked against the same E
        stub().with_coord_diff(torch.zeros((3, 3)))


def test_h_of_another_size_is_a_value_error_at_the_call():
    net = EGCL(5, 5, 32)
    el = stub(n=3, cd=torch.zeros((2, 3)))
    for call in (net, net.forward_edges):
        with torch.no_grad(), pytest.raises(ValueError, match="4 nodes .* prepared for 3"):
            call(torch.zeros((4, 5)), el)
    with pytest.raises(ValueError, match="prepared for 3"):    # with grad as well: before any refusal of autograd
        net.forward_edges(torch.zeros((4, 5), requires_grad=True), el)
    with torch.no_grad(), pytest.raises(ValueError, match="with_coord_diff"):
        net(torch.zeros((3, 5)), stub(n=3))


def test_limits_raise_the_plain_lists_not_implemented_error():
    row, col = torch.tensor([0, 1]), torch.tensor([1, 2])
    with pytest.raises(NotImplementedError, match="4194304 nodes and fewer than 2\\^31 - 1024 edges"):
        EdgeList(row, col, num_nodes=4194305)
    big = torch.empty((1 << 31) - 1024, dtype=torch.int32, device="meta")
    with pytest.raises(NotImplementedError, match=r"got 7 nodes, 2147482624 edges"):
        EdgeList(big, big, num_nodes=7)
    import inspect
    assert "takes up to 4194304 nodes and fewer than 2^31 - 1024" in inspect.getsource(EGCL._infer_list)


def test_cpu_tensors_are_refused():
    row, col, cd = torch.tensor([0, 1]), torch.tensor([1, 2]), torch.zeros((2, 3))
    with pytest.raises(_lib.HipPathError):
        EdgeList(row, col, cd, num_nodes=3)
    with pytest.raises(_lib.HipPathError):
        EdgeList(row, col, num_nodes=3)
    with pytest.raises(_lib.HipPathError):
        stub().with_coord_diff(cd)
    net = EGCL(5, 5, 32)
    with torch.no_grad(), pytest.raises(_lib.HipPathError):
        net(torch.zeros((3, 5)), stub(cd=cd))
    with pytest.raises(_lib.HipPathError):
        net.forward_edges(torch.zeros((3, 5), requires_grad=True), stub(cd=cd))


def test_wide_layers_refuse_the_handle_with_the_list_text():
    net = EGCL(5, 5, 256)
    with torch.no_grad(), pytest.raises(NotImplementedError, match="up to hidden_nf 128; at hidden_nf 256 pass the"):
        net(torch.zeros((3, 5)), stub(cd=torch.zeros((2, 3))))
    with pytest.raises(NotImplementedError, match="up to hidden_nf 128"):
        net.forward_edges(torch.zeros((3, 5)), stub(cd=torch.zeros((2, 3))))


# ---------------------------------------------------------------------------
# (c) the C entries
# ---------------------------------------------------------------------------
def test_entries_declared_and_bound_with_the_headers_argument_count():
    protos = header_prototypes()
    for name, nargs in ENTRIES.items():
        assert name in protos, f"{name} is not declared in include/enflow_hip.h"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
        assert len(_lib.SIGNATURES[name][1]) == protos[name] == nargs, name


@pytest.mark.parametrize("nf", [None, 16], ids=["libenflow_hip", "libenflow_hip_nf16"])
def test_entries_exported_and_argument_errors_launch_nothing(nf):
    L = _lib.lib(nf)
    assert L.enflow_abi_version() == 13   # additive exports: no ABI bump
    for name in ENTRIES:
        assert hasattr(L, name), name
    assert L.enflow_graph_sort_tile() == SORT_TILE
    size = L.enflow_graph_workspace_size
    assert size(-1, 0) == -1 and size(0, -1) == -1
    assert size((1 << 22) + 1, 4) == -3 and size(4, (1 << 31) - 1024) == -3
    assert 0 < size(0, 0) == size(1 << 22, 0) < size(5, 1) <= size(5, 512) < size(5, 513)
    per_edge = (size(100, 2_000_000) - size(100, 1_000_000)) / 1e6
    assert 13.9 < per_edge < 14.1, per_edge           # two key arrays, one of values, 256 counters per 512 edges
    one = 8   # a non-null pointer that is never dereferenced: every check comes before any launch
    csr = lambda n=49, E=100, rb=8, cb=8, p=None, ws=None, wsb=1 << 40: L.enflow_graph_csr_build(   # noqa: E731
        n, E, p, rb, p, cb, p, p, p, p, ws, wsb, None)
    csc = lambda n=49, E=100, p=None, ws=None, wsb=1 << 40: L.enflow_graph_csc_build(n, E, p, p, p, ws, wsb, None)   # noqa: E731
    for call in (csr, csc):
        assert call() == -1                                  # null pointers
        assert call(n=-1) == -1 and call(E=-1) == -1
        assert call(n=(1 << 22) + 1) == -3 and call(n=1 << 22) == -1
        assert call(E=(1 << 31) - 1024) == -3
        assert call(p=one, ws=one, wsb=size(49, 100) - 1) == -6
        assert call(n=0, E=0) == -1                          # null pointers come before the empty batch
        assert call(n=0, E=0, p=one, ws=one) == 0            # no nodes: nothing is launched
    assert csr(rb=2, p=one, ws=one) == -1 and csr(cb=16, p=one, ws=one) == -1
    gather = lambda E=100, eb=4, p=None: L.enflow_graph_gather_f32(E, p, eb, p, p, None)      # noqa: E731
    scatter = lambda E=100, eb=4, p=None: L.enflow_graph_scatter_f32(E, p, p, p, eb, None)    # noqa: E731
    for call in (gather, scatter):
        assert call() == -1 and call(E=-1) == -1 and call(eb=2, p=one) == -1
        assert call(E=(1 << 31) - 1024, p=one) == -3
        assert call(E=0) == 0 and call(E=0, eb=8) == 0       # nothing to move: pointers may be null


# ---------------------------------------------------------------------------
# (d) what the build must return
# ---------------------------------------------------------------------------
def csr_numpy(n, row, col):
    """(row_ptr, col sorted and clamped, order, bad_row) of a list: a stable sort
    of the rows clamped to [0, n), col clamped to [-1, n] before the int32 cast."""
    row, col = np.asarray(row, dtype=np.int64), np.asarray(col, dtype=np.int64)
    rc = np.clip(row, 0, n - 1)
    order = np.argsort(rc, kind="stable")
    ptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(rc, minlength=n), out=ptr[1:])
    return ptr, np.clip(col, -1, n)[order].astype(np.int32), order, bool((rc != row).any())


@pytest.mark.parametrize("kind", GRAPHS)
def test_numpy_statement_matches_csc_numpy_and_the_torch_builders(kind):
    rng = np.random.RandomState(11)
    n, row, col = graph(kind, rng)
    if row.size:
        perm = rng.permutation(row.size)
        row, col = row[perm], col[perm]
    ptr, colp, order, bad = csr_numpy(n, row, col)
    row_ptr, tcol, _, torder, tbad = EGCL._list_csr(n, torch.tensor(row), torch.tensor(col), torch.zeros((row.size, 3)))
    assert np.array_equal(row_ptr.numpy(), ptr) and np.array_equal(tcol.numpy(), colp)
    assert np.array_equal(torder.numpy(), order) and bool(tbad) == bad is False
    # the CSC of the sorted list is a CSR build keyed by its col
    cptr, _, cperm, _ = csr_numpy(n, colp, colp)
    want_ptr, want_perm = csc_numpy(n, colp)
    assert np.array_equal(cptr, want_ptr) and np.array_equal(cperm, want_perm)
    col_ptr, col_perm = EGCL._list_csc(n, tcol)
    assert np.array_equal(col_ptr.numpy(), cptr) and np.array_equal(col_perm.numpy(), cperm)


def test_numpy_statement_clamps_like_the_torch_builder():
    n = 6
    row = np.array([2, -1, 6, 0, 5, 2 ** 32 + 1], dtype=np.int64)
    col = np.array([-1, 6, 2 ** 32 + 3, -7, 0, 5], dtype=np.int64)
    ptr, colp, order, bad = csr_numpy(n, row, col)
    row_ptr, tcol, _, torder, tbad = EGCL._list_csr(n, torch.tensor(row), torch.tensor(col), torch.zeros((6, 3)))
    assert bad and bool(tbad)
    assert np.array_equal(row_ptr.numpy(), ptr) and np.array_equal(torder.numpy(), order)
    assert np.array_equal(tcol.numpy(), colp) and set(colp.tolist()) == {-1, 0, 5, 6}   # 2^32 + 3 did not wrap to 3
