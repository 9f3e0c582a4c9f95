"""Shared by tests/test_edge_list_grad_host.py and tests/test_gpu_edge_list_grad.py:
a torch restatement of enflow/nn/egcl.py:57-92 on (row, col, coord_diff) built
from an EGCL module's own Sequentials (float64 is the reference every GPU
gradient is compared against, float32 its floor), the synthetic graphs, a numpy
restatement of the CSC view, and the weighted-sum loss that puts random
adjoints on Q, F and G."""
import copy

import numpy as np
import torch


class List:
    """A duck-typed edge list: what the reference's EGCL.forward reads."""

    def __init__(self, row, col, coord_diff):
        self.row, self.col, self.coord_diff = row, col, coord_diff


def weighted(outs, weights):
    """sum_k (w_k * out_k).sum() over the outputs whose weight is not None."""
    terms = [(w * o).sum() for o, w in zip(outs, weights) if w is not None]
    return sum(terms[1:], terms[0])


def restate_forward(m, h, row, col, cd):
    """egcl.py:57-92 with the module's own edge_nn / att_nn / coord_nn / node_nn /
    vel_scaling_nn, on whatever dtype and device the arguments have."""
    n = h.shape[0]
    radial = (cd ** 2).sum(1).unsqueeze(1)                              # egcl.py:80
    cdn = cd / (torch.sqrt(radial) + 1) if m.norm_diff else cd          # egcl.py:82-84
    e = m.edge_nn(torch.cat([h[row], h[col], radial], 1))               # egcl.py:57-59
    if m.attention:
        e = e * m.att_nn(e)                                             # egcl.py:60-62
    trans = torch.clamp(cdn * m.coord_nn(e), min=-100, max=100)         # egcl.py:72-73
    i3 = row.unsqueeze(1).expand(-1, 3)
    fs = torch.zeros(n, 3, dtype=h.dtype).scatter_add(0, i3, trans)
    cnt = torch.zeros(n, 3, dtype=h.dtype).scatter_add(0, i3, torch.ones_like(trans))
    F = fs / cnt.clamp(min=1) * m.coords_weight                         # helpers.py:63-70, egcl.py:75
    agg = torch.zeros(n, e.shape[1], dtype=h.dtype).scatter_add(0, row.unsqueeze(1).expand(-1, e.shape[1]), e)
    G = m.node_nn(torch.cat([h, agg], 1))                               # egcl.py:65-69
    return m.vel_scaling_nn(h), F, G


def restate(net, h, row, col, cd, weights, dtype=torch.float64):
    """Outputs and gradients of the restatement on the CPU in `dtype`.  h, cd:
    numpy or tensors (any dtype; they are rounded to float32 first, what the
    device is fed); weights: (wQ, wF, wG) numpy arrays or None.  Returns
    (outs {Q, F, G}, grads {h, coord_diff, <parameter names>}), numpy float64;
    parameters without a gradient in the graph (a partial upstream) give zeros,
    act_fn's own parameters (a frozen PReLU slope) are left out."""
    # a CPU copy of the module in `dtype` (EGCL(tanh=True) holds a non-leaf tensor: no deepcopy of the whole)
    m = type(net)(net.input_nf, net.output_nf, net.hidden_nf, act_fn=copy.deepcopy(net.act_fn).cpu(),
                  coords_weight=net.coords_weight, attention=net.attention, norm_diff=net.norm_diff, tanh=net.tanh)
    m.load_state_dict({k: v.detach().cpu() for k, v in net.state_dict().items()})
    m = m.to(dtype)
    own = {id(p) for p in m.act_fn.parameters()}
    for p in m.parameters():
        p.requires_grad_(id(p) not in own)
        p.grad = None
    as_t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float32)).to(dtype)   # noqa: E731
    h = as_t(h).requires_grad_(True)
    cd = as_t(cd).reshape(-1, 3).requires_grad_(True)
    row = torch.as_tensor(np.asarray(row, dtype=np.int64))
    col = torch.as_tensor(np.asarray(col, dtype=np.int64))
    outs = restate_forward(m, h, row, col, cd)
    w = [None if x is None else as_t(x) for x in weights]
    weighted(outs, w).backward()
    z = lambda t: np.zeros(tuple(t.shape)) if t.grad is None else t.grad.double().numpy()   # noqa: E731
    grads = {"h": z(h), "coord_diff": z(cd)}
    grads.update({k: z(p) for k, p in m.named_parameters() if id(p) not in own})
    return {k: o.detach().double().numpy() for k, o in zip("QFG", outs)}, grads


def scatter_to_pos(n, row, col, dcd):
    """d pos of coord_diff = pos[row] - pos[col]: + on row, - on col."""
    out = np.zeros((n, 3))
    np.add.at(out, np.asarray(row), dcd)
    np.add.at(out, np.asarray(col), -dcd)
    return out


def csc_numpy(n, col):
    """(col_ptr, col_perm) of a list: per column, its edges in increasing index."""
    col = np.asarray(col, dtype=np.int64)
    ptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(col, minlength=n), out=ptr[1:])
    perm = np.concatenate([np.nonzero(col == c)[0] for c in range(n)]) if col.size else np.zeros(0, np.int64)
    return ptr, perm


def rand_cd(rng, E):
    """coord_diff entries uniform in +-[0.3, 2]: order 1, no |cd| near 0."""
    return (rng.uniform(0.3, 2.0, (E, 3)) * rng.choice([-1.0, 1.0], (E, 3))).astype(np.float32)


def graph(kind, rng):
    """(n, row, col) of a synthetic graph: the smallest that reaches its code path."""
    if kind == "n1_no_edges":
        return 1, np.zeros(0, np.int64), np.zeros(0, np.int64)
    if kind == "n40_no_edges":                # two row blocks, E == 0
        return 40, np.zeros(0, np.int64), np.zeros(0, np.int64)
    if kind == "n33_two_blocks_empty_rows":   # second block: one row, without edges; so is row 5
        row = np.repeat([r for r in range(33) if r not in (5, 32)], 3)
        return 33, row, rng.randint(0, 33, row.size)
    if kind == "row_of_200_edges":            # spans pair tiles and wave slabs
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
    if kind == "column_only_and_never_column":   # node 4 only receives, node 0 never does
        return 5, np.array([0, 0, 1, 2, 3, 1]), np.array([4, 1, 4, 3, 2, 4])
    if kind == "hub":                         # 70 nodes in three row blocks, 16 duplicates each to node 0
        return 70, np.repeat(np.arange(70), 16), np.zeros(70 * 16, np.int64)
    if kind == "random_20":
        row = rng.randint(0, 20, 90)
        return 20, row, rng.randint(0, 20, 90)
    raise KeyError(kind)


GRAPHS = ["n1_no_edges", "n40_no_edges", "n33_two_blocks_empty_rows", "row_of_200_edges", "two_passes_1280_edges",
          "columns_in_other_blocks", "repeats_and_self_loops", "column_only_and_never_column", "hub", "random_20"]


def case_inputs(kind, nf, seed=11):
    """(n, row, col, cd, h) of a synthetic case, the list shuffled (the host sorts it)."""
    rng = np.random.RandomState(seed)
    n, row, col = graph(kind, rng)
    E = row.size
    if E:
        perm = rng.permutation(E)
        row, col = row[perm], col[perm]
    cd = rand_cd(rng, E)
    h = rng.uniform(-1.0, 1.0, (n, nf)).astype(np.float32)
    return n, row, col, cd, h


def rand_weights(n, out_nf, seed=3):
    rng = np.random.RandomState(seed)
    return (rng.uniform(-1, 1, (n, 1)).astype(np.float32), rng.uniform(-1, 1, (n, 3)).astype(np.float32),
            rng.uniform(-1, 1, (n, out_nf)).astype(np.float32))
