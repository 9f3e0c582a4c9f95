"""Float64 torch restatement of LFIntegrator.reverse (enflow/flow/dynamics.py:25-37)
with the per-molecule log|detJ| of its continuous layers -- TEST HELPER, not collected.

Built from the gradient oracle's EGCL and pbc (oracle.enflow_oracle_grad._egcl /
_pbc) and the oracle's edge builder (oracle.enflow_oracle.batch_edges): the
neighbour lists are integer outputs and carry no gradient, as in the reference,
which differentiates through Edges.coord_diff only.  ``restate`` leaves autograd
history on its outputs; ``recurrence`` is the hand-written adjoint of one
reverse layer applied layer by layer (the EGCL vjp alone comes from autograd),
the recurrence the HIP backward implements.
"""
import numpy as np
import torch

from oracle import enflow_oracle as O
from oracle.enflow_oracle_grad import _egcl, _pbc

KEYS = ("h", "g", "pos", "vel")


def _t(a, dtype):
    return torch.tensor(np.asarray(a, dtype=np.float64)).to(dtype)


def _mol_index(mol_ptr):
    mol_ptr = np.asarray(mol_ptr, dtype=np.int64)
    return torch.as_tensor(np.repeat(np.arange(len(mol_ptr) - 1), np.diff(mol_ptr)), dtype=torch.long)


def _edges(pos, state):
    row, col, eb = O.batch_edges(pos.detach().double().numpy(), np.asarray(state["box"], dtype=np.float64),
                                 np.asarray(state["r_cut"], dtype=np.float64),
                                 np.asarray(state["mol_ptr"], dtype=np.int64))
    return torch.as_tensor(row, dtype=torch.long), torch.as_tensor(col, dtype=torch.long), eb


def _params(layers, dtype, grad=True):
    return [{k: _t(v, dtype).requires_grad_(grad) for k, v in p.items() if k not in ("flags", "act")}
            for p in layers]


def restate(layers, state, dt, coords_weight=1.0, dtype=torch.float64):
    """The continuous layers of the reverse on leaf tensors.  Returns (out, P,
    leaves): out = dict(h, g, pos, vel, ldj) with autograd history -- ldj
    [num_mols] = minus the sum of Q over the molecule's atoms and layers -- the
    layers' leaf parameter dicts and the leaf inputs dict(h, g, pos, vel)."""
    P = _params(layers, dtype)
    leaves = {k: _t(state[k], dtype).requires_grad_(True) for k in KEYS}
    box = _t(state["box"], dtype)
    mol = _mol_index(state["mol_ptr"])
    M = len(state["mol_ptr"]) - 1
    h, g, pos, vel = (leaves[k] for k in KEYS)
    n = h.shape[0]
    ldj = torch.zeros(M, dtype=dtype)
    for p, lp in zip(reversed(P), reversed(layers)):
        h = h - g * dt
        pos = _pbc(pos - vel * dt, box)
        row, col, eb = _edges(pos, state)
        q, f, gg = _egcl(p, h, pos, row, col, _t(eb, dtype), n, coords_weight, lp.get("flags", (0, 0, 0)),
                         lp.get("act"))
        g = g - gg * dt
        vel = (vel - f * dt) / torch.exp(q)
        ldj = ldj.index_add(0, mol, -q.reshape(-1))
    return dict(h=h, g=g, pos=pos, vel=vel, ldj=ldj), P, leaves


def weights(shapes, seed):
    """The fixed random weights of the test loss: dict name -> float64 array."""
    rng = np.random.default_rng(seed)
    return {k: rng.normal(size=s) for k, s in shapes.items()}


def loss_of(out, w, dtype=None):
    """sum_k <w_k, out_k> over the names in w."""
    tot = 0.0
    for k, wk in w.items():
        o = out[k]
        tot = tot + (o * torch.as_tensor(wk).to(device=o.device, dtype=o.dtype if dtype is None else dtype)).sum()
    return tot


def grads_of(loss, P, leaves):
    """float64 numpy gradients ([layer dicts], input dict); unreached leaves get zeros."""
    flat = [v for p in P for v in p.values()] + list(leaves.values())
    gs = torch.autograd.grad(loss, flat, allow_unused=True)
    gs = [torch.zeros_like(v) if g is None else g for v, g in zip(flat, gs)]
    it = iter(gs)
    gl = [{k: next(it).double().numpy() for k in p} for p in P]
    gi = {k: next(it).double().numpy() for k in leaves}
    return gl, gi


def reference(layers, state, dt, w, coords_weight=1.0, dtype=torch.float64):
    """Values and gradients of loss_of(restate(...), w): (out numpy dict, [layer
    grad dicts], input grad dict)."""
    out, P, leaves = restate(layers, state, dt, coords_weight, dtype)
    gl, gi = grads_of(loss_of(out, w), P, leaves)
    return {k: v.detach().double().numpy() for k, v in out.items()}, gl, gi


def recurrence(layers, state, dt, w, coords_weight=1.0):
    """The same gradients without autograd over the flow: the float64 reverse
    with a state tape (h', x', v', Q per layer), then per layer, first layer
    last:  aG = -dt ag';  aF = -dt exp(-Q) av';  aQ = -(v' . av') - a_ldj[mol];
    (dh', dx', parameter gradients) = EGCL vjp at (h', x');  ah = ah' + dh';
    ax = ax' + dx';  ag = ag' - dt ah;  av = exp(-Q) av' - dt ax."""
    dtype = torch.float64
    box = _t(state["box"], dtype)
    mol = _mol_index(state["mol_ptr"])
    h, g, pos, vel = (_t(state[k], dtype) for k in KEYS)
    n = h.shape[0]
    tape = {}
    with torch.no_grad():
        P0 = _params(layers, dtype, grad=False)
        for l in reversed(range(len(layers))):
            h = h - g * dt
            pos = _pbc(pos - vel * dt, box)
            row, col, eb = _edges(pos, state)
            q, f, gg = _egcl(P0[l], h, pos, row, col, _t(eb, dtype), n, coords_weight,
                             layers[l].get("flags", (0, 0, 0)), layers[l].get("act"))
            g = g - gg * dt
            vel = (vel - f * dt) / torch.exp(q)
            tape[l] = (h, pos, vel, q, row, col, eb)
    zero = lambda k, ref: _t(w[k], dtype) if k in w else torch.zeros_like(ref)  # noqa: E731
    ah, ag, ax, av = zero("h", h), zero("g", g), zero("pos", pos), zero("vel", vel)
    aldj = zero("ldj", torch.zeros(len(state["mol_ptr"]) - 1, dtype=dtype))
    gl = [None] * len(layers)
    for l in range(len(layers)):
        hl, xl, vl, q, row, col, eb = tape[l]
        e = torch.exp(-q)
        aG = -dt * ag
        aF = -dt * e * av
        aQ = -(vl * av).sum(1, keepdim=True) - aldj[mol].reshape(-1, 1)
        p = {k: v.clone().requires_grad_(True) for k, v in P0[l].items()}
        hh, xx = hl.clone().requires_grad_(True), xl.clone().requires_grad_(True)
        Q, F, G = _egcl(p, hh, xx, row, col, _t(eb, dtype), n, coords_weight, layers[l].get("flags", (0, 0, 0)),
                        layers[l].get("act"))
        names = list(p)
        gs = torch.autograd.grad([Q, F, G], [hh, xx] + [p[k] for k in names], [aQ, aF, aG], allow_unused=True)
        dh, dx = gs[0], gs[1]
        gl[l] = {k: (torch.zeros_like(p[k]) if gk is None else gk).numpy() for k, gk in zip(names, gs[2:])}
        ah = ah + dh
        ax = ax + dx
        ag = ag - dt * ah
        av = e * av - dt * ax
    return gl, dict(h=ah.numpy(), g=ag.numpy(), pos=ax.numpy(), vel=av.numpy())


def model_layers(model):
    """The oracle's layer dicts of an enflow_amd LFIntegrator (float64)."""
    from _fixtures import EGCL_KEYS, ATT_KEYS
    out = []
    for n in model.networks:
        keep = EGCL_KEYS + (ATT_KEYS if n.attention else ())
        p = {k: v.detach().cpu().double().numpy() for k, v in n.state_dict().items() if k in keep}
        p["flags"] = (bool(n.attention), bool(n.norm_diff), bool(n.tanh))
        p["act"] = tuple(float(x) for x in n.act())     # (kind, p0, p1), the oracle's numbering
        out.append(p)
    return out
