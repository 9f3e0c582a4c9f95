"""Per-molecule energies and negative log-likelihoods with their gradients --
TEST HELPER, not collected.

``restate`` is enflow/flow/loss.py:11-24 in torch for each molecule as a batch
of one (the reference's own arithmetic: triu of the squared distances, zero
entries dropped, r^2 = d^2 + softening, 4 (1 / r^12 - 1 / r^6)), on leaf
tensors so that autograd gives the reference gradients.  ``closed_form`` is the
formula the HIP backward implements, in numpy without autograd.  ``batch`` /
``upstreams`` build the inputs the CPU and the GPU tests share, ``reference``
the float64 values and gradients (cached) after the float32 floor check.
"""
import math

import numpy as np
import torch

from _fixtures import normwise

KEYS = ("h", "g", "pos", "vel")
FLOATS = KEYS + ("box", "r_cut")
VAL_TOL = 1e-5       # values: per element, relative to the sum of absolute terms
GRAD_TOL = 5e-5      # gradients: normwise per tensor
PF = 10.0
L2PI = math.log(2.0 * math.pi)


def kBT():
    from enflow_amd.data.synthetic import default_kBT
    return float(default_kBT())


def f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


# ---------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------
_BATCHES = {}


def batch(sizes, seed, nf=5, coincident=()):
    """A ragged batch (float32-representable float64 arrays; cached, never
    modified).  Batches with a molecule past 256 atoms are LJ boxes.
    coincident: (molecule, i, j) triples -- atom i is moved onto atom j."""
    key = (tuple(sizes), seed, nf, tuple(coincident))
    if key not in _BATCHES:
        from enflow_amd.data.synthetic import make_molecules, make_lj_systems
        if max(sizes) > 256:
            b = make_lj_systems(list(sizes), nf=nf, seed=seed)
        else:
            b = make_molecules(len(sizes), list(sizes), nf=nf, seed=seed)
            # continuous features, as a flow's output has them
            b["h"] = b["h"] + 0.3 * np.random.default_rng(seed + 1000).normal(size=b["h"].shape)
        for k in FLOATS:
            b[k] = f32(b[k])
        for m, i, j in coincident:
            a0 = int(b["mol_ptr"][m])
            b["pos"][a0 + i] = b["pos"][a0 + j]
        _BATCHES[key] = b
    return _BATCHES[key]


def upstreams(M, seed=7):
    """The fixed random [M] upstream gradients of a batch, each with a zero and
    a negative entry (float32-representable).  Three molecules or more: one
    vector, zero at M // 2, the last entry negative.  Two molecules: two
    vectors, (-a, 0) and (0, -b), so that each molecule is weighted once."""
    w = np.abs(np.random.default_rng(seed).normal(size=M)) + 0.25
    assert M >= 2
    if M == 2:
        return [f32(np.array([-w[0], 0.0])), f32(np.array([0.0, -w[1]]))]
    w[-1] = -w[-1]
    w[M // 2] = 0.0
    return [f32(w)]


def ldj_of(M, seed=8):
    return f32(np.random.default_rng(seed).normal(scale=20.0, size=M))


# ---------------------------------------------------------------------------
# loss.py per molecule, in torch
# ---------------------------------------------------------------------------
def lj_torch(pos, softening):
    """_get_lj_potential of one molecule (loss.py:14-18)."""
    dist_sq = torch.triu((pos.unsqueeze(1) - pos).pow(2).sum(dim=2))
    r_sq = dist_sq[dist_sq != 0] + softening
    r_6 = r_sq.pow(3)
    r_12 = r_6.pow(2)
    return 4 * (1 / r_12 - 1 / r_6).sum()


def nll_torch(h, g, pos, vel, ldj, kbt, softening, pf=PF):
    """__call__ of one molecule as a batch of one (loss.py:21-24)."""
    H = lj_torch(pos, softening) + 0.5 * (vel ** 2).sum()
    logZ = -pos.shape[0] * (math.log(pf) - 1.5 * math.log(2 * math.pi / kbt))
    lg = lambda z: -0.5 * ((z ** 2).sum() + L2PI)  # noqa: E731
    return -(-H / kbt + logZ + ldj + lg(h) + lg(g))


def restate(b, ldj, kbt, softening, pf=PF, dtype=torch.float64):
    """(pot [M], nll [M], leaves): the per-molecule values with autograd history
    on the leaf tensors dict(h, g, pos, vel, ldj)."""
    leaves = {k: torch.tensor(np.asarray(b[k], dtype=np.float64)).to(dtype).requires_grad_(True) for k in KEYS}
    leaves["ldj"] = torch.tensor(np.asarray(ldj, dtype=np.float64)).to(dtype).requires_grad_(True)
    ptr = [int(x) for x in b["mol_ptr"]]
    pot, nll = [], []
    for m in range(len(ptr) - 1):
        s = slice(ptr[m], ptr[m + 1])
        pot.append(lj_torch(leaves["pos"][s], softening) + 0 * leaves["pos"][s].sum())
        nll.append(nll_torch(leaves["h"][s], leaves["g"][s], leaves["pos"][s], leaves["vel"][s], leaves["ldj"][m],
                             kbt, softening, pf))
    return torch.stack(pot), torch.stack(nll), leaves


def grads(vals, w, leaves):
    """numpy float64 gradients of <w, vals> w.r.t. every leaf (zeros where unreached)."""
    wt = torch.as_tensor(np.asarray(w, dtype=np.float64)).to(vals.dtype)
    names = list(leaves)
    gs = torch.autograd.grad((vals * wt).sum(), [leaves[k] for k in names], allow_unused=True, retain_graph=True)
    return {k: (np.zeros(tuple(leaves[k].shape)) if gk is None else gk.double().numpy()) for k, gk in zip(names, gs)}


# ---------------------------------------------------------------------------
# the formula the kernels implement, numpy
# ---------------------------------------------------------------------------
def lj_force(pos, softening):
    """dLJ / dpos [n][3] of one molecule: sum over b != a of dE/dr^2 * 2 (pos_a -
    pos_b), dE/dr^2 = 4 (3 r^-8 - 6 r^-14) in r^2 = d^2 + softening; d^2 == 0 dropped."""
    pos = np.asarray(pos, dtype=np.float64)
    d = pos[:, None, :] - pos[None, :, :]
    d2 = np.sum(d * d, axis=2)
    keep = d2 != 0
    r = np.where(keep, d2 + softening, 1.0)
    f = np.where(keep, 8.0 * (3.0 / r ** 4 - 6.0 / r ** 7), 0.0)
    return np.sum(f[:, :, None] * d, axis=1)


def closed_form(b, w, coef, softening):
    """dict(h, g, pos, vel) of the adjoints for upstream w [M] and coef [4]."""
    out = {k: np.zeros_like(np.asarray(b[k], dtype=np.float64)) for k in KEYS}
    ptr = [int(x) for x in b["mol_ptr"]]
    for m in range(len(ptr) - 1):
        s = slice(ptr[m], ptr[m + 1])
        out["pos"][s] = w[m] * coef[0] * lj_force(b["pos"][s], softening)
        out["vel"][s] = 2.0 * w[m] * coef[1] * b["vel"][s]
        out["h"][s] = 2.0 * w[m] * coef[2] * b["h"][s]
        out["g"][s] = 2.0 * w[m] * coef[3] * b["g"][s]
    return out


def coefs(kbt):
    return (1.0, 0.0, 0.0, 0.0), (1.0 / kbt, 0.5 / kbt, 0.5, 0.5)


# ---------------------------------------------------------------------------
# scales and bars
# ---------------------------------------------------------------------------
def lj_abs(pos, softening):
    """Sum over i < j pairs of |4 r^-12| + |4 r^-6| (the terms the energy sums)."""
    pos = np.asarray(pos, dtype=np.float64)
    d2 = np.triu(np.sum((pos[:, None, :] - pos[None, :, :]) ** 2, axis=2))
    r6 = (d2[d2 != 0] + softening) ** 3
    return float(np.sum(4.0 / r6 ** 2 + 4.0 / r6))


def scales(b, ldj, kbt, softening, pf=PF):
    """(potS [M], nllS [M]): the sums of the absolute values of each element's terms."""
    ptr = [int(x) for x in b["mol_ptr"]]
    M = len(ptr) - 1
    potS, nllS = np.zeros(M), np.zeros(M)
    for m in range(M):
        s = slice(ptr[m], ptr[m + 1])
        n = ptr[m + 1] - ptr[m]
        potS[m] = lj_abs(b["pos"][s], softening)
        logZ = -n * (math.log(pf) - 1.5 * math.log(2 * math.pi / kbt))
        nllS[m] = (potS[m] + 0.5 * np.sum(b["vel"][s] ** 2)) / kbt + abs(logZ) + abs(ldj[m]) + \
            0.5 * np.sum(b["h"][s] ** 2) + 0.5 * np.sum(b["g"][s] ** 2) + L2PI
    return potS, nllS


def value_errs(got, ref, S):
    """Worst |got - ref| / S_m over the elements with S_m > 0; elements with no
    term at all (a molecule without a pair) must be exactly the reference's."""
    got, ref, S = (np.atleast_1d(np.asarray(x, dtype=np.float64)) for x in (got, ref, S))
    assert np.all(np.isfinite(got)), "non-finite values"
    assert np.array_equal(got[S == 0], ref[S == 0])
    return float(np.max(np.abs(got - ref)[S > 0] / S[S > 0])) if np.any(S > 0) else 0.0


def grad_errs(got, ref):
    """{tensor: normwise error}; a tensor that is exactly zero in the reference must be exactly zero."""
    out = {}
    for k, r in ref.items():
        if k not in got:
            continue
        if np.linalg.norm(r) == 0:
            assert not np.any(got[k]), f"{k} is exactly zero in the reference"
            continue
        out[k] = normwise(got[k], r)
    return out


_REF = {}


def reference(b, key, softening, wi=0):
    """float64 reference of a batch with its upstream vector number wi (cached):
    dict with pot, nll [M], potS, nllS, w, ldj, gpot / gnll (gradient dicts of
    <w, pot> / <w, nll>), after asserting that the float32 restatement stays
    within HALF of each bar."""
    key = (key, softening, wi)
    if key in _REF:
        return _REF[key]
    kbt = kBT()
    M = len(b["mol_ptr"]) - 1
    w = upstreams(M)[wi]
    ldj = ldj_of(M)
    pot, nll, leaves = restate(b, ldj, kbt, softening)
    r = dict(w=w, ldj=ldj, kBT=kbt, pot=pot.detach().numpy(), nll=nll.detach().numpy(),
             gpot=grads(pot, w, leaves), gnll=grads(nll, w, leaves))
    r["potS"], r["nllS"] = scales(b, ldj, kbt, softening)
    p32, n32, l32 = restate(b, ldj, kbt, softening, dtype=torch.float32)
    floor = {"pot": value_errs(p32.detach().numpy(), r["pot"], r["potS"]),
             "nll": value_errs(n32.detach().numpy(), r["nll"], r["nllS"])}
    gfloor = {f"pot.{k}": v for k, v in grad_errs(grads(p32, w, l32), r["gpot"]).items()}
    gfloor.update({f"nll.{k}": v for k, v in grad_errs(grads(n32, w, l32), r["gnll"]).items()})
    print(f"{key}: float32 restatement vs float64: values {floor}, worst gradient "
          f"{max(gfloor.values()) if gfloor else 0.0:.2e}")
    assert all(v <= VAL_TOL / 2 for v in floor.values()), f"{key}: the float32 floor exceeds half the value bar: {floor}"
    assert all(v <= GRAD_TOL / 2 for v in gfloor.values()), \
        f"{key}: the float32 floor exceeds half the gradient bar: {gfloor}"
    r["floor"], r["gfloor"] = floor, gfloor
    _REF[key] = r
    return r


# the batches of tests/test_gpu_energy_grad.py: name -> (sizes, seed, nf, coincident, softenings)
GPU_BATCHES = {
    "n32": ((1, 2, 5, 22, 32), 101, 5, (), (0.1, 0.0)),
    "n64": ((33, 64), 102, 5, (), (0.1,)),
    "n256": ((65, 256, 3), 103, 5, (), (0.1,)),
    "lj": ((300, 7), 104, 5, (), (0.1,)),
    "coincident32": ((2, 5, 22), 105, 5, ((0, 1, 0), (1, 3, 0), (2, 21, 4)), (0.0, 0.1)),
    "coincident_lj": ((300, 2), 106, 5, ((0, 17, 250), (1, 1, 0)), (0.0, 0.1)),
    "nf12": ((5, 22, 40), 107, 12, (), (0.1,)),
}


def gpu_batch(name):
    sizes, seed, nf, co, _ = GPU_BATCHES[name]
    return batch(sizes, seed, nf=nf, coincident=co)


def references(name, softening):
    """The batch and its references, one per upstream vector."""
    b = gpu_batch(name)
    return b, [reference(b, name, softening, wi) for wi in range(len(upstreams(len(b["mol_ptr"]) - 1)))]
