"""Golden flow at hidden_nf 256 from the REFERENCE's own modules in float64.

Run where the reference is present (see make_golden.py):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_wide.py

``LFIntegrator(EGCL(5, 5, 256) x 2, ArgMax(5, 256))`` on a 5 + 9 + 22-atom
batch: forward outputs, log|detJ|, the NLL and the reverse of the forward
output.  Two 256-wide layers hold ~400 k weights, more than a committed
fixture may: the file stores the torch seed instead, and per parameter its
sum, sum of squares and first four values, so a test that rebuilds the
modules from the seed (same construction order: the layers, then the ArgMax)
can tell that it holds the reference's weights.  Writes
tests/golden/lf_h256_L2.npz: inputs float32-representable, outputs float64.
"""
import numpy as np
import torch

import make_golden as G
from make_golden import Alchemical_NLL, ArgMax, EGCL, LFIntegrator, batch_inputs, default_dt, default_kBT, ref_data, save

HID, N_LAYERS, NF, SIZES, SEED = 256, 2, 5, [5, 9, 22], 256


def fingerprint(module, prefix):
    out = {}
    for k, v in module.state_dict().items():
        w = v.detach().numpy().astype(np.float32).astype(np.float64).reshape(-1)   # as the float32 the tests rebuild
        out[f"{prefix}{k}.fp"] = np.concatenate([[w.sum(), (w * w).sum()], w[:4], np.zeros(max(0, 4 - w.size))])
    return out


def case():
    torch.manual_seed(SEED)
    dt = default_dt()
    nets = [EGCL(NF, NF, HID) for _ in range(N_LAYERS)]
    am = ArgMax(NF, HID)
    fp = {}
    for i, net in enumerate(nets):
        fp.update(fingerprint(net, f"p{i}."))
    fp.update(fingerprint(am, "dq."))
    model = LFIntegrator(nets, am, dt=dt)   # BaseFlow casts to float64
    # the tests rebuild float32 weights: run the reference on exactly those values
    with torch.no_grad():
        for p in model.parameters():
            p.copy_(p.to(torch.float32).to(torch.float64))
    b = batch_inputs(len(SIZES), SIZES, NF, seed=SEED)
    d = ref_data(b)
    torch.manual_seed(SEED + 1)
    eps = torch.randn(d.h.size())
    torch.manual_seed(SEED + 1)
    with torch.no_grad():
        out, ldj = model(d)
    kBT = default_kBT()
    with torch.no_grad():
        loss = Alchemical_NLL(kBT=kBT, softening=0.1)(out, ldj)
    res = {"h": out.h.numpy().copy(), "g": out.g.numpy().copy(), "pos": out.pos.numpy().copy(),
           "vel": out.vel.numpy().copy(), "ldj": float(ldj), "nll": float(loss)}
    with torch.no_grad():
        back = model.reverse(out)
    res.update({"rev_h": back.h.numpy(), "rev_g": back.g.numpy(), "rev_pos": back.pos.numpy(),
                "rev_vel": back.vel.numpy()})
    inp = dict(b)
    inp.update(eps=eps.numpy(), dt=np.array(dt), kBT=np.array(kBT), softening=np.array(0.1),
               n_layers=np.array(N_LAYERS), hid=np.array(HID), seed=np.array(SEED))
    res.update(fp)
    save("lf_h256_L2", inp, res)


if __name__ == "__main__":
    assert G.REPO
    case()
