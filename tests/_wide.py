"""Shared helpers of the hidden_nf 129..256 tests (test_wide_hidden_host.py,
test_gpu_wide_hidden.py): the width-256 golden's model rebuilt from its seed,
oracle parameter dicts of enflow_amd modules, batches."""
import numpy as np
import torch

from _fixtures import load

GOLDEN = "lf_h256_L2"


def oracle_params(mod, dtype=np.float64):
    """The oracle's parameter dict of an enflow_amd EGCL / ArgMax."""
    from enflow_amd.nn import EGCL
    p = {k: v.detach().cpu().numpy().astype(dtype) for k, v in mod.state_dict().items()}
    code = mod.act()
    if int(code[0]) != 0:
        p["act"] = tuple(float(x) for x in code)
    if isinstance(mod, EGCL):
        p["flags"] = (mod.attention, mod.norm_diff, mod.tanh)
    return p


def fingerprint(t):
    w = t.detach().cpu().numpy().astype(np.float64).reshape(-1)
    return np.concatenate([[w.sum(), (w * w).sum()], w[:4], np.zeros(max(0, 4 - w.size))])


def golden_model(device="cpu"):
    """(model, inp, out): the golden's LFIntegrator rebuilt from its torch seed
    in the reference's construction order (the layers, then the ArgMax), checked
    against the stored per-parameter fingerprints."""
    from enflow_amd.nn import EGCL, ArgMax
    from enflow_amd.flow import LFIntegrator
    inp, out = load(GOLDEN)
    hid, nf, nl = int(inp["hid"]), inp["h"].shape[1], int(inp["n_layers"])
    torch.manual_seed(int(inp["seed"]))
    nets = [EGCL(nf, nf, hid) for _ in range(nl)]
    am = ArgMax(nf, hid)
    for i, m in list(enumerate(nets)) + [("dq", am)]:
        pre = "dq." if i == "dq" else f"p{i}."
        for k, v in m.state_dict().items():
            np.testing.assert_allclose(fingerprint(v), out[f"{pre}{k}.fp"], rtol=1e-12, atol=0, err_msg=pre + k)
    model = LFIntegrator(nets, am, dt=float(inp["dt"])).to(device)
    return model, inp, out


def f32(b):
    o = dict(b)
    for k in ("h", "g", "pos", "vel", "box", "r_cut"):
        o[k] = np.asarray(b[k]).astype(np.float32).astype(np.float64)
    return o


def cast(b, dtype):
    o = dict(b)
    for k in ("h", "g", "pos", "vel", "box", "r_cut"):
        o[k] = np.asarray(b[k]).astype(dtype)
    return o
