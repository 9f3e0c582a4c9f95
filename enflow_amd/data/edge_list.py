"""A prepared edge list: the caller's (row, col, coord_diff) with the CSR the
edge-list kernels read built once, on the device (enflow_graph_csr_build), and
reused by every call -- EGCL.forward under no_grad, EGCL.forward_edges and its
backward, which adds the CSC view (enflow_graph_csc_build) the first time it
runs.  What is left per call is the gather of coord_diff into the sorted order
and, in the backward, the scatter of d coord_diff back.

    el = EdgeList(row, col, coord_diff, num_nodes=n)
    q, f, g = layer.forward_edges(h, el)
    el2 = el.with_coord_diff(new_cd)      # same topology object, nothing rebuilt

``EdgeList`` is not an ``Edges``: it carries row, col and coord_diff as the
caller gave them and is accepted wherever such an object is.  The topology is
keyed by (data_ptr, _version) of row and col, like the packed-weight caches: an
in-place change of either rebuilds it at the next use.  Nothing here reads the
device: a row outside [0, num_nodes) sets a device word that the forward ORs
into the error word it reads anyway (IndexError there, like the plain list).
"""
import torch

from .. import _lib

MAX_NODES = 4194304
MAX_EDGES = (1 << 31) - 1024    # exclusive


def _limits(n, E):
    if n > MAX_NODES or E >= MAX_EDGES:
        raise NotImplementedError("the edge-list EGCL kernel takes up to 4194304 nodes and fewer than 2^31 - 1024 "
                                  f"edges (got {n} nodes, {E} edges)")


def _index_bytes(t, what):
    if t.dtype == torch.int32:
        return 4
    if t.dtype == torch.int64:
        return 8
    raise ValueError(f"EdgeList {what} must be int32 or int64 (got {t.dtype})")


class Topology:
    """(row, col, num_nodes) and what the kernels read of it.  Shared by every
    with_coord_diff sibling; rebuilt in place when row or col changed."""

    def __init__(self, row, col, num_nodes):
        self.row, self.col, self.num_nodes = row, col, int(num_nodes)
        self.num_edges = int(row.numel())
        self.builds = 0          # CSR builds so far (tests and tools read it)
        self._key = None
        self._csr = None
        self._csc = None
        self.csr()

    def _current_key(self):
        return (self.row.data_ptr(), self.row._version, self.col.data_ptr(), self.col._version)

    def _workspace(self, L, dev):
        need = L.enflow_graph_workspace_size(self.num_nodes, self.num_edges)
        if need < 0:
            raise _lib.HipPathError(f"enflow_graph_workspace_size failed with code {need}")
        return torch.empty(max(need, 1), dtype=torch.uint8, device=dev)

    def csr(self):
        """(row_ptr [n + 1] int32, col [E] int32 sorted and clamped, order [E]
        int32, bad_row [1] int32: ERR_INDEX if a row was clamped), built on the
        current stream; cached until row or col change."""
        key = self._current_key()
        if self._csr is not None and self._key == key:
            return self._csr
        L = _lib.lib()
        n, E = self.num_nodes, self.num_edges
        row, col = self.row.reshape(-1), self.col.reshape(-1)
        if not row.is_contiguous():
            row = row.contiguous()
        if not col.is_contiguous():
            col = col.contiguous()
        dev = row.device
        row_ptr = torch.empty(n + 1, dtype=torch.int32, device=dev)
        colp = torch.empty(E, dtype=torch.int32, device=dev)
        order = torch.empty(E, dtype=torch.int32, device=dev)
        bad = torch.zeros(1, dtype=torch.int32, device=dev)
        if n == 0:
            row_ptr.zero_()
        ws = self._workspace(L, dev)
        _lib.check(L.enflow_graph_csr_build(n, E, _lib.ptr(row), _index_bytes(row, "row"), _lib.ptr(col),
                                            _index_bytes(col, "col"), _lib.ptr(row_ptr), _lib.ptr(colp),
                                            _lib.ptr(order), _lib.ptr(bad), _lib.ptr(ws), ws.numel(),
                                            _lib.stream_ptr(dev)), "enflow_graph_csr_build")
        self._csr, self._csc, self._key = (row_ptr, colp, order, bad), None, key
        self.builds += 1
        return self._csr

    def csc(self):
        """(col_ptr [n + 1] int32, col_perm [E] int32) of the current CSR, built
        the first time a backward asks for it."""
        row_ptr, colp, order, _ = self.csr()
        if self._csc is not None:
            return self._csc
        L = _lib.lib()
        n, E = self.num_nodes, self.num_edges
        dev = colp.device
        col_ptr = torch.empty(n + 1, dtype=torch.int32, device=dev)
        col_perm = torch.empty(E, dtype=torch.int32, device=dev)
        if n == 0:
            col_ptr.zero_()
        ws = self._workspace(L, dev)
        _lib.check(L.enflow_graph_csc_build(n, E, _lib.ptr(colp), _lib.ptr(col_ptr), _lib.ptr(col_perm), _lib.ptr(ws),
                                            ws.numel(), _lib.stream_ptr(dev)), "enflow_graph_csc_build")
        self._csc = (col_ptr, col_perm)
        return self._csc

    def gather(self, coord_diff):
        """coord_diff [E, 3] (fp32 / fp64, the caller's order) -> contiguous fp32 in the sorted order."""
        order = self.csr()[2]
        E = self.num_edges
        if coord_diff.dtype not in (torch.float32, torch.float64):
            coord_diff = coord_diff.to(torch.float32)
        cd = coord_diff.contiguous()
        out = torch.empty((E, 3), dtype=torch.float32, device=cd.device)
        _lib.check(_lib.lib().enflow_graph_gather_f32(E, _lib.ptr(cd), cd.element_size(), _lib.ptr(order),
                                                      _lib.ptr(out), _lib.stream_ptr(cd.device)),
                   "enflow_graph_gather_f32")
        return out

    def scatter(self, sorted_grad, dtype):
        """d coord_diff [E, 3] fp32 in the sorted order -> the caller's order, in `dtype`."""
        order = self.csr()[2]
        E = self.num_edges
        via = dtype if dtype in (torch.float32, torch.float64) else torch.float32
        out = torch.empty((E, 3), dtype=via, device=sorted_grad.device)
        _lib.check(_lib.lib().enflow_graph_scatter_f32(E, _lib.ptr(sorted_grad), _lib.ptr(order), _lib.ptr(out),
                                                       out.element_size(), _lib.stream_ptr(out.device)),
                   "enflow_graph_scatter_f32")
        return out.to(dtype)


class EdgeList:
    """row, col [E] (int32 / int64) and coord_diff [E, 3] (fp32 / fp64, or None
    until with_coord_diff) on the GPU, over num_nodes nodes; the CSR is built
    here, on the current stream, without a device-to-host read."""

    def __init__(self, row, col, coord_diff=None, num_nodes=None, _topology=None):
        # shapes first, then the kernels' limits, then the device: each refusal is the same on any machine
        if _topology is None:
            if num_nodes is None:
                raise ValueError("EdgeList needs num_nodes (deriving it from row / col would read the device)")
            if not (isinstance(row, torch.Tensor) and isinstance(col, torch.Tensor)):
                raise TypeError("EdgeList expects row and col tensors")
            n = int(num_nodes)
            E = int(row.numel())
            if n < 0:
                raise ValueError(f"EdgeList of {n} nodes")
            if col.numel() != E:
                raise ValueError(f"edge list of {E} rows with {col.numel()} cols")
            _index_bytes(row, "row"), _index_bytes(col, "col")
            self._check_cd(coord_diff, E)
            _limits(n, E)
            for t in (row, col) + (() if coord_diff is None else (coord_diff,)):
                _lib.require_gpu(t)
            _topology = Topology(row, col, n)
        else:
            self._check_cd(coord_diff, _topology.num_edges)
            if coord_diff is not None:
                _lib.require_gpu(coord_diff)
        self.topology = _topology
        self.coord_diff = coord_diff

    @staticmethod
    def _check_cd(coord_diff, E):
        if coord_diff is not None and tuple(coord_diff.shape) != (E, 3):
            raise ValueError(f"edge list of {E} rows with coord_diff {tuple(coord_diff.shape)}")

    @property
    def row(self):
        return self.topology.row

    @property
    def col(self):
        return self.topology.col

    @property
    def num_nodes(self):
        return self.topology.num_nodes

    @property
    def num_edges(self):
        return self.topology.num_edges

    def with_coord_diff(self, coord_diff):
        """The same edges with another coord_diff: shares this handle's topology (nothing is rebuilt)."""
        return EdgeList(None, None, coord_diff, _topology=self.topology)
