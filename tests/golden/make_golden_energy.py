"""Golden per-molecule energies, negative log-likelihoods and their gradients
from the REFERENCE's own Alchemical_NLL (enflow/flow/loss.py) in float64.

Run where the reference is present (see make_golden.py):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_energy.py

Every molecule of a batch is run as a batch of ONE through the reference's
``_get_lj_potential`` and ``__call__`` (with that molecule's ``ldj``), and
autograd gives the gradients w.r.t. pos / vel / h / g.  Molecules of 1, 2, 5 and
22 atoms plus a 5-atom molecule whose atoms 3 and 0 coincide; softening 0.1 and
0.  Writes tests/golden/energy_grad_s01.npz and energy_grad_s0.npz: inputs
float32-representable (stored float32), outputs float64.
"""
import numpy as np
import torch

import make_golden as G      # the reference's modules, RefData and the batch helpers
from make_golden import Alchemical_NLL, RefData, batch_inputs, default_kBT, f32, save, to_t

SIZES = [1, 2, 5, 22, 5]
COINCIDENT = (4, 3, 0)       # molecule 4: atom 3 sits on atom 0
PF = 10.0


def inputs(seed=71):
    b = batch_inputs(len(SIZES), SIZES, 5, seed, one_hot=False)
    m, i, j = COINCIDENT
    a0 = int(b["mol_ptr"][m])
    b["pos"][a0 + i] = b["pos"][a0 + j]
    b["ldj"] = f32(np.random.default_rng(seed + 1).normal(scale=20.0, size=len(SIZES)))
    return b


def one_molecule(b, m):
    s = slice(int(b["mol_ptr"][m]), int(b["mol_ptr"][m + 1]))
    leaf = {k: to_t(b[k][s]).requires_grad_(True) for k in ("h", "g", "pos", "vel")}
    d = RefData(leaf["h"], leaf["g"], leaf["pos"], leaf["vel"], to_t(b["box"][s]), to_t(b["r_cut"][m:m + 1]),
                torch.tensor([s.stop - s.start]))
    return d, leaf


def case(softening, name):
    b = inputs()
    kBT = float(default_kBT())
    nll = Alchemical_NLL(kBT=kBT, partition_func=PF, softening=softening)
    M, A = len(SIZES), int(b["mol_ptr"][-1])
    out = dict(pot=np.zeros(M), nll=np.zeros(M), dpot_pos=np.zeros((A, 3)))
    out.update({f"dnll_{k}": np.zeros_like(b[k]) for k in ("h", "g", "pos", "vel")})
    for m in range(M):
        s = slice(int(b["mol_ptr"][m]), int(b["mol_ptr"][m + 1]))
        d, leaf = one_molecule(b, m)
        pot = nll._get_lj_potential(d)
        out["pot"][m] = float(pot.detach())
        if torch.is_tensor(pot) and pot.requires_grad:
            out["dpot_pos"][s] = torch.autograd.grad(pot, leaf["pos"])[0].numpy()
        d, leaf = one_molecule(b, m)
        val = nll(d, to_t(b["ldj"][m]))
        out["nll"][m] = float(val.detach())
        gs = torch.autograd.grad(val, [leaf[k] for k in ("h", "g", "pos", "vel")], allow_unused=True)
        for k, gk in zip(("h", "g", "pos", "vel"), gs):
            if gk is not None:
                out[f"dnll_{k}"][s] = gk.numpy()
    inp = {k: b[k] for k in ("h", "g", "pos", "vel", "box", "r_cut", "mol_ptr", "ldj")}
    inp.update(kBT=np.float64(kBT), softening=np.float64(softening), partition_func=np.float64(PF))
    save(name, inp, out)


if __name__ == "__main__":
    assert G.REPO
    case(0.1, "energy_grad_s01")
    case(0.0, "energy_grad_s0")
