"""CPU-only checks behind the edge-list EGCL backward (tests/test_gpu_edge_list_grad.py):

(a) the float64 torch restatement of egcl.py:57-92 on (row, col, coord_diff), built
    from the module's own Sequentials, that every GPU gradient is compared against:
    its outputs against oracle.enflow_oracle.egcl_forward, its gradients against
    oracle.enflow_oracle_grad._egcl on a list derived from positions in a box large
    enough that coord_diff = pos[row] - pos[col] (d pos = the scatter of d coord_diff);
(b) the CSC builder against a numpy restatement on the synthetic graphs;
(c) the new C entries: declared, bound, exported, their argument-error codes, and
    workspace sizes monotone;
(d) the refusal text of EGCL.forward on a list still names no_grad and Data.edges."""
import re

import numpy as np
import pytest
import torch
from torch import nn

from oracle import enflow_oracle as O
from oracle import enflow_oracle_grad as OG
from _fixtures import normwise
from _edge_list_grad import (List, GRAPHS, case_inputs, csc_numpy, graph, rand_weights, restate, scatter_to_pos,
                             weighted)
from test_edge_list_egcl_host import header_prototypes
from enflow_amd import _lib
from enflow_amd.nn import EGCL


def module(seed, nf_in=5, nf_out=5, hid=32, **kw):
    torch.manual_seed(seed)
    return EGCL(nf_in, nf_out, hid, **kw)


def oracle_params(net):
    p = {k: v.detach().double().numpy() for k, v in net.state_dict().items()}
    p["flags"] = (net.attention, net.norm_diff, net.tanh)
    return p


# ---------------------------------------------------------------------------
# (a) the restatement
# ---------------------------------------------------------------------------
VARIANTS = [dict(), dict(attention=True, norm_diff=True, tanh=True), dict(nf_out=3), dict(coords_weight=0.5)]


@pytest.mark.parametrize("kw", VARIANTS, ids=["default", "all_flags", "5_to_3", "coords_weight"])
def test_restatement_outputs_match_the_numpy_oracle(kw):
    net = module(1, **kw)
    n, row, col, cd, h = case_inputs("random_20", net.input_nf)
    outs, _ = restate(net, h, row, col, cd, rand_weights(n, net.output_nf))
    want = O.egcl_forward(oracle_params(net), h.astype(np.float64), row, col, cd.astype(np.float64),
                          coords_weight=net.coords_weight)
    for k, w in zip("QFG", want):
        assert normwise(outs[k], w) < 1e-12, k


@pytest.mark.parametrize("kw", VARIANTS[:2], ids=["default", "all_flags"])
def test_restatement_gradients_match_the_gradient_oracle(kw):
    net = module(2, **kw)
    rng = np.random.RandomState(4)
    n, row, col = graph("random_20", rng)
    pos = (rng.randint(0, 129, (n, 3)) / 64.0).astype(np.float32)   # a grid: the differences are exact in fp32
    keep = np.abs(pos[row] - pos[col]).max(1) > 0.05          # norm_diff: no |coord_diff| at 0
    row, col = row[keep], col[keep]
    h = rng.uniform(-1, 1, (n, 5)).astype(np.float32)
    w = rand_weights(n, 5)
    cd = pos[row].astype(np.float64) - pos[col].astype(np.float64)
    assert np.array_equal(cd.astype(np.float32).astype(np.float64), cd)
    _, got = restate(net, h, row, col, cd.astype(np.float32), w)
    # the gradient oracle on the positions; its box (100) never wraps these differences
    p = {k: torch.tensor(v.detach().double().numpy(), requires_grad=True) for k, v in net.state_dict().items()}
    ht = torch.tensor(h, dtype=torch.float64, requires_grad=True)
    pt = torch.tensor(pos, dtype=torch.float64, requires_grad=True)
    r, c = torch.tensor(row), torch.tensor(col)
    outs = OG._egcl(p, ht, pt, r, c, torch.full((row.size, 3), 100.0, dtype=torch.float64), n, 1.0,
                    flags=(net.attention, net.norm_diff, net.tanh))
    weighted(outs, [torch.tensor(x, dtype=torch.float64) for x in w]).backward()
    tol = 1e-12
    assert normwise(got["h"], ht.grad.numpy()) < tol
    assert normwise(scatter_to_pos(n, row, col, got["coord_diff"]), pt.grad.numpy()) < tol
    for k, v in p.items():
        assert normwise(got[k], v.grad.numpy()) < tol, k


def test_restatement_leaves_a_frozen_prelu_slope_out():
    net = module(3, act_fn=nn.PReLU(init=0.2))
    for q in net.act_fn.parameters():
        q.requires_grad_(False)
    n, row, col, cd, h = case_inputs("random_20", 5)
    _, grads = restate(net, h, row, col, cd, rand_weights(n, 5))
    assert "edge_nn.1.weight" not in grads and "edge_nn.0.weight" in grads


# ---------------------------------------------------------------------------
# (b) the CSC view
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", GRAPHS)
def test_csc_builder_matches_numpy(kind):
    rng = np.random.RandomState(11)
    n, row, col = graph(kind, rng)
    if row.size:
        perm = rng.permutation(row.size)
        row, col = row[perm], col[perm]
    cd = torch.zeros((row.size, 3))
    row_ptr, colp, _, order, bad = EGCL._list_csr(n, torch.tensor(row), torch.tensor(col), cd)
    assert not bool(bad)
    order = order.numpy()
    assert np.array_equal(np.sort(order), np.arange(row.size))
    assert np.all(np.diff(row[order]) >= 0) and np.array_equal(colp.numpy(), col[order])
    same_row = np.diff(row[order]) == 0
    assert np.all(np.diff(order)[same_row] > 0)                       # stable
    assert np.array_equal(row_ptr.numpy(), np.concatenate([[0], np.cumsum(np.bincount(row, minlength=n))]))
    col_ptr, col_perm = EGCL._list_csc(n, colp)
    want_ptr, want_perm = csc_numpy(n, col[order])
    assert col_ptr.dtype == torch.int32 and col_perm.dtype == torch.int32
    assert np.array_equal(col_ptr.numpy(), want_ptr) and np.array_equal(col_perm.numpy(), want_perm)
    if kind == "hub":
        assert want_ptr[1] - want_ptr[0] == row.size >= 1100           # one column, every edge
    if kind == "column_only_and_never_column":
        assert 4 not in row and 4 in col and 0 not in col


# ---------------------------------------------------------------------------
# (c) the C entries
# ---------------------------------------------------------------------------
FWD, SIZE, BWD = ("enflow_egcl_forward_list_tape_f32", "enflow_egcl_backward_list_workspace_size",
                  "enflow_egcl_backward_list_f32")


def test_entries_declared_and_bound_with_the_headers_argument_count():
    protos = header_prototypes()
    for name, nargs in ((FWD, 17), (SIZE, 4), (BWD, 25)):
        assert name in protos, f"{name} is not declared in include/enflow_hip.h"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
        assert len(_lib.SIGNATURES[name][1]) == protos[name] == nargs, name


def fwd(L, n=49, E=100, nf=5, H=128, prec=_lib.PREC_F32):
    return L.enflow_egcl_forward_list_tape_f32(n, E, nf, H, None, None, None, None, None, 1.0, None, None, None, None,
                                               prec, None, None)


def bwd(L, n=49, E=100, nf=5, H=128, flags=_lib.BWD_F32, wsb=1 << 40):
    return L.enflow_egcl_backward_list_f32(n, E, nf, H, *([None] * 9), flags, 1.0, *([None] * 7), wsb, None, None)


@pytest.mark.parametrize("nf", [None, 16], ids=["libenflow_hip", "libenflow_hip_nf16"])
def test_entries_exported_and_argument_errors_launch_nothing(nf):
    L = _lib.lib(nf)
    assert L.enflow_abi_version() == 13   # additive exports: no ABI bump
    width = L.enflow_max_node_nf()
    for name in (FWD, SIZE, BWD):
        assert hasattr(L, name)
    size = L.enflow_egcl_backward_list_workspace_size
    for call in (fwd, bwd):                # every pointer null: whatever it returns, it launched nothing
        assert call(L) == -1
        assert call(L, n=-1) == -1 and call(L, E=-1) == -1
        assert call(L, nf=0) == -4 and call(L, nf=width + 1) == -4 and call(L, nf=width) == -1
        assert call(L, H=48) == -5 and call(L, H=256) == -5
        assert call(L, n=(1 << 22) + 1) == -3 and call(L, n=1 << 22) == -1
        assert call(L, E=(1 << 31) - 1024) == -3
        assert call(L, n=0, E=0) == -1     # null pointers come before the empty batch
    assert fwd(L, prec=_lib.PREC_BF16) == -1 and fwd(L, prec=3) == -1
    assert fwd(L, prec=_lib.PREC_F16X3 | _lib.EGCL_VARIANTS) == -1
    assert bwd(L, flags=0x400) == -1                                    # an unknown flag bit
    assert size(-1, 0, 5, 128) == -1 and size(4, -1, 5, 128) == -1
    assert size(4, 4, 0, 128) == -4 and size(4, 4, width + 1, 128) == -4
    assert size(4, 4, 5, 48) == -5
    assert size((1 << 22) + 1, 4, 5, 128) == -3 and size(4, (1 << 31) - 1024, 5, 128) == -3
    assert size(1 << 22, (1 << 31) - 2048, 5, 128) == -3                # more than 2^31 - 1 pair rows
    # sizes: monotone in nodes, edges and the hidden width; about 1.6 KB per edge at H = 128 (8-feature library)
    assert 0 < size(0, 0, 5, 32) <= size(49, 0, 5, 32) < size(49, 100, 5, 32) < size(49, 101, 5, 32)
    assert size(49, 100, 5, 32) <= size(50, 100, 5, 32) < size(200, 100, 5, 32)   # node rows come in 64-float lines
    assert size(50, 100, 5, 32) < size(50, 100, 5, 64) < size(50, 100, 5, 128)
    per_edge = (size(1000, 2_000_000, 5, 128) - size(1000, 1_000_000, 5, 128)) / 1e6
    assert 1500 < per_edge < (1800 if width == 8 else 1900), per_edge


def test_backward_workspace_too_small_is_minus_6():
    L = _lib.lib(None)
    need = L.enflow_egcl_backward_list_workspace_size(49, 100, 5, 128)
    one = 8   # a non-null pointer that is never dereferenced: the size is checked before any launch
    args = lambda wsb: (49, 100, 5, 128, *([one] * 9), _lib.BWD_F32, 1.0, *([one] * 7), wsb, one, None)   # noqa: E731
    assert L.enflow_egcl_backward_list_f32(*args(need - 1)) == -6
    assert L.enflow_egcl_backward_list_f32(*args(0)) == -6


# ---------------------------------------------------------------------------
# (d) the refusal of EGCL.forward on a list, and forward_edges' argument checks
# ---------------------------------------------------------------------------
def test_refusal_text_names_no_grad_data_edges_and_forward_edges():
    import inspect
    src = inspect.getsource(EGCL._forward_list)
    msg = " ".join(re.findall(r'"([^"]*)"', src[src.index("raise NotImplementedError"):]))
    for word in ("no_grad", "Data.edges", "forward_edges"):
        assert word in msg, (word, msg)


def test_forward_edges_refuses_cpu_tensors_and_non_lists():
    net = EGCL(5, 5, 32)
    h = torch.zeros((3, 5), requires_grad=True)
    edges = List(torch.tensor([0, 1]), torch.tensor([1, 2]), torch.zeros((2, 3)))
    with pytest.raises(_lib.HipPathError):
        net.forward_edges(h, edges)
    for bad in (None, (torch.tensor([0]), torch.tensor([1])), torch.zeros((2, 1), dtype=torch.long)):
        with pytest.raises(TypeError):
            net.forward_edges(h, bad)
