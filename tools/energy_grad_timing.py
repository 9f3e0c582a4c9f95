"""Time one energy-training step  reverse_grad -> loss -> backward()  with the
energy from (a) Alchemical_NLL.potential_grad and (b) the torch pair potential
on top of reverse_grad, the only route before potential_grad existed: (b1) per
molecule in a Python loop, as tests/test_gpu_reverse_grad.py composes it, and
(b2) the same arithmetic batched over equal-size molecules.  Loss:
mean(U / kBT - rev_ldj).  One process, alternating windows, three per path,
host clock around a final synchronise; then the per-kernel split of one step
(a) from the library's event timer, with the share of the new kernels.

    python tools/energy_grad_timing.py [--mols 1024] [--atoms 22] [--layers 8] [--hid 128] [--out FILE.json]
    python tools/energy_grad_timing.py --lj 2944 --iters 3 [--out FILE.json]      (one LJ box, no dequantiser)

Prints a table and one JSON line; needs the GPU.  Numbers for DESIGN.md only (no bars).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def lj_loop(pos, mol_ptr, soft):
    """[M] energies, one molecule at a time (loss.py:11-19 in torch)."""
    out = []
    for m in range(len(mol_ptr) - 1):
        x = pos[mol_ptr[m]:mol_ptr[m + 1]]
        d2 = torch.triu((x.unsqueeze(1) - x).pow(2).sum(2))
        r6 = (d2[d2 != 0] + soft).pow(3)
        out.append(4 * (1 / r6.pow(2) - 1 / r6).sum())
    return torch.stack(out)


def lj_batched(pos, M, n, soft):
    """The same for M molecules of n atoms each, without the loop."""
    x = pos.reshape(M, n, 3)
    d2 = torch.triu((x.unsqueeze(2) - x.unsqueeze(1)).pow(2).sum(3))
    keep = d2 != 0
    r6 = (torch.where(keep, d2, torch.ones_like(d2)) + soft).pow(3)
    return torch.where(keep, 4 * (1 / r6.pow(2) - 1 / r6), torch.zeros_like(d2)).sum((1, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mols", type=int, default=1024)
    ap.add_argument("--atoms", type=int, default=22)
    ap.add_argument("--lj", type=int, default=0, help="one LJ box of this many atoms instead of the molecules")
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--hid", type=int, default=128)
    ap.add_argument("--nf", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from enflow_amd import _lib
    from enflow_amd.nn import EGCL, ArgMax
    from enflow_amd.flow import LFIntegrator, Alchemical_NLL
    from enflow_amd.data import Data
    from enflow_amd.data.synthetic import make_molecules, make_lj_systems, default_dt, default_kBT
    dev = "cuda:0"
    torch.manual_seed(0)
    if a.lj:
        b = make_lj_systems(a.lj, nf=a.nf, seed=1)
        M, n, dq = 1, a.lj, None
    else:
        b = make_molecules(a.mols, a.atoms, nf=a.nf, seed=1)
        M, n, dq = a.mols, a.atoms, ArgMax(a.nf, a.hid)
    model = LFIntegrator([EGCL(a.nf, a.nf, a.hid) for _ in range(a.layers)], dq, dt=default_dt()).to(dev)
    data = Data.from_arrays(b, device=dev)
    kBT, soft = float(default_kBT()), 0.1
    nll = Alchemical_NLL(kBT=kBT, softening=soft)
    ptr = [int(x) for x in b["mol_ptr"]]
    last = {}

    def step(energy, name):
        model.zero_grad(set_to_none=True)
        out, ldj = model.reverse_grad(data.clone())
        loss = (energy(out) / kBT - ldj).mean()
        loss.backward()
        last[name] = loss

    paths = {"(a) potential_grad": lambda: step(nll.potential_grad, "a"),
             "(b1) torch pair potential, per-molecule loop": lambda: step(lambda o: lj_loop(o.pos, ptr, soft), "b1"),
             "(b2) torch pair potential, batched": lambda: step(lambda o: lj_batched(o.pos, M, n, soft), "b2")}
    for f in paths.values():       # warm-up: allocator, packed weights, instance selection
        for _ in range(2):
            f()
    torch.cuda.synchronize()
    losses = {k: float(v.detach()) for k, v in last.items()}
    ms = {k: [] for k in paths}
    for _ in range(3):             # alternating windows
        for k, f in paths.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.iters):
                f()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3 / a.iters)
    with _lib.KernelTimer() as kt:
        paths["(a) potential_grad"]()
        torch.cuda.synchronize()
    split = {k: {"ms": v[0], "launches": v[1]} for k, v in sorted(kt.stats.items(), key=lambda kv: -kv[1][0])}
    total = sum(v["ms"] for v in split.values())
    new = sum(v["ms"] for k, v in split.items() if k.startswith("nll_mol_bwd"))
    fwd = sum(v["ms"] for k, v in split.items() if k == "nll_mol_kernel")
    shape = f"one {a.lj}-atom LJ box" if a.lj else f"{a.mols} x {a.atoms} atoms"
    print(f"{shape}, {a.layers} layers, H {a.hid}, nf {a.nf}; ms per step, three windows of {a.iters}; losses {losses}")
    for k, v in ms.items():
        print(f"  {k:46s} " + "  ".join(f"{x:9.3f}" for x in v) + f"   median {np.median(v):9.3f}")
    print(f"per-kernel split of one step (a) (event timer, {total:.3f} ms of the library's kernels):")
    for k, v in split.items():
        print(f"  {k:36s} {v['ms']:8.3f} ms  {v['launches']:4d} launches  {100 * v['ms'] / max(total, 1e-9):5.1f} %")
    step_ms = float(np.median(ms["(a) potential_grad"]))
    print(f"new backward kernel nll_mol_bwd_kernel: {new:.4f} ms = {100 * new / max(total, 1e-9):.2f} % of the library's "
          f"kernel time, {100 * new / step_ms:.2f} % of the step; the energy's forward nll_mol_kernel: {fwd:.4f} ms")
    line = {"shape": {k: v for k, v in vars(a).items() if k != "out"}, "losses": losses, "ms_per_step": ms,
            "kernel_split": split, "kernel_ms_total": total, "nll_mol_bwd_ms": new, "nll_mol_fwd_ms": fwd}
    print(json.dumps(line))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(line, fh, indent=1)


if __name__ == "__main__":
    main()
