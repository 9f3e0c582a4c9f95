"""Time LFIntegrator.reverse_grad + backward() against the likelihood training
step (forward + Alchemical_NLL + backward) and the inference
reverse(return_ldj=True), in one process: alternating windows, three per
path, host clock around a final synchronise; then the per-kernel split of one
reverse_grad + backward from the library's event timer (with the share of the
two glue kernels lf_rev_adj_pre / lf_rev_adj_post).

    python tools/reverse_grad_timing.py [--mols 1024] [--atoms 22] [--layers 8] [--hid 128] [--out FILE.json]

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mols", type=int, default=1024)
    ap.add_argument("--atoms", type=int, default=22)
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
    from enflow_amd.data.synthetic import make_molecules, default_dt, default_kBT
    dev = "cuda:0"
    torch.manual_seed(0)
    model = LFIntegrator([EGCL(a.nf, a.nf, a.hid) for _ in range(a.layers)], ArgMax(a.nf, a.hid),
                         dt=default_dt()).to(dev)
    b = make_molecules(a.mols, a.atoms, nf=a.nf, seed=1)
    data = Data.from_arrays(b, device=dev)
    noise = torch.randn(b["h"].shape, device=dev)
    nll = Alchemical_NLL(kBT=default_kBT(), softening=0.1)
    w = torch.randn(b["pos"].shape, device=dev)

    def energy_step():
        model.zero_grad(set_to_none=True)
        out, ldj = model.reverse_grad(data.clone())
        ((out.pos * w).sum() - ldj.sum()).backward()

    def nll_step():
        model.zero_grad(set_to_none=True)
        out, ldj = model(data.clone(), noise=noise)
        nll(out, ldj).backward()

    def infer():
        with torch.no_grad():
            model.reverse(data.clone(), return_ldj=True)

    paths = {"reverse_grad + backward": energy_step, "forward + NLL + backward": nll_step,
             "reverse(return_ldj=True), no_grad": infer}
    for f in paths.values():       # warm-up: allocator, packed weights, instance selection
        for _ in range(3):
            f()
    torch.cuda.synchronize()
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
        energy_step()
        torch.cuda.synchronize()
    split = {k: {"ms": v[0], "launches": v[1]} for k, v in sorted(kt.stats.items(), key=lambda kv: -kv[1][0])}
    total = sum(v["ms"] for v in split.values())
    glue = sum(v["ms"] for k, v in split.items() if k.startswith("lf_rev_adj_"))
    print(f"{a.mols} x {a.atoms} atoms, {a.layers} layers, H {a.hid}, nf {a.nf}; ms per call, three windows of {a.iters}")
    for k, v in ms.items():
        print(f"  {k:36s} " + "  ".join(f"{x:8.3f}" for x in v) + f"   median {np.median(v):8.3f}")
    print(f"per-kernel split of one reverse_grad + backward (event timer, {total:.3f} ms of kernels):")
    for k, v in split.items():
        print(f"  {k:36s} {v['ms']:8.3f} ms  {v['launches']:4d} launches  {100 * v['ms'] / max(total, 1e-9):5.1f} %")
    print(f"glue kernels lf_rev_adj_pre + lf_rev_adj_post: {glue:.3f} ms = {100 * glue / max(total, 1e-9):.2f} % of kernel time")
    line = {"shape": {k: v for k, v in vars(a).items() if k != "out"},"ms_per_call": ms, "kernel_split": split, "kernel_ms_total": total, "glue_ms": glue}
    print(json.dumps(line))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(line, fh, indent=1)


if __name__ == "__main__":
    main()
