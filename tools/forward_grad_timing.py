"""Time one likelihood-training step two ways: (a) the plain step  forward ->
nll -> backward()  and (b) the per-molecule-weighted step  forward_grad ->
(w * nll.per_molecule_grad(out, ldj_mol)).sum() -> backward().  With
--parent-lib (a) also runs against another build of the library (the parent
commit's), alternating with this tree's in the same process: (a) on this tree
must sit inside the window-to-window scatter the parent shows against itself.
One process, alternating windows, host clock around a final synchronise.

    python tools/forward_grad_timing.py [--mols 1024] [--atoms 22] [--layers 8] [--hid 128]
                                        [--parent-lib PATH/libenflow_hip.so] [--out FILE.json]

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
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from enflow_amd import _lib
    from enflow_amd.nn import EGCL, ArgMax
    from enflow_amd.flow import LFIntegrator, Alchemical_NLL
    from enflow_amd.data import Data
    from enflow_amd.data.synthetic import make_molecules, default_dt, default_kBT
    dev = "cuda:0"
    torch.manual_seed(0)
    b = make_molecules(a.mols, a.atoms, nf=a.nf, seed=1)
    model = LFIntegrator([EGCL(a.nf, a.nf, a.hid) for _ in range(a.layers)], ArgMax(a.nf, a.hid), dt=default_dt()).to(dev)
    data = Data.from_arrays(b, device=dev)
    noise = torch.randn_like(data.h)
    nll = Alchemical_NLL(kBT=float(default_kBT()), softening=0.1)
    w = torch.softmax(torch.randn(a.mols, device=dev), 0)
    this_lib = _lib.LIB_PATH
    last = {}

    def use(path):
        if _lib.LIB_PATH != path or not _lib._libs:
            _lib._libs.clear()
            _lib.LIB_PATH = path
            for mod in model.modules():      # packed buffers belong to the library that packed them
                for attr in ("_packed_key", "_layers_key", "_train_key"):
                    if hasattr(mod, attr):
                        setattr(mod, attr, None)

    def plain(path, name):
        use(path)
        model.zero_grad(set_to_none=True)
        out, ldj = model(data.clone(), noise=noise)
        loss = nll(out, ldj)
        loss.backward()
        last[name] = loss

    def weighted():
        use(this_lib)
        model.zero_grad(set_to_none=True)
        out, ldj_mol = model.forward_grad(data.clone(), noise=noise)
        loss = (w * nll.per_molecule_grad(out, ldj_mol)).sum()
        loss.backward()
        last["b"] = loss

    paths = {"(a) forward + nll, this tree": lambda: plain(this_lib, "a")}
    if a.parent_lib:
        paths["(a) forward + nll, parent library"] = lambda: plain(os.path.abspath(a.parent_lib), "a_parent")
    paths["(b) forward_grad + weighted per_molecule_grad"] = weighted
    for f in paths.values():       # warm-up: allocator, packed weights, code objects
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    losses = {k: float(v.detach()) for k, v in last.items()}
    ms = {k: [] for k in paths}
    for _ in range(a.windows):     # alternating windows
        for k, f in paths.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.iters):
                f()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3 / a.iters)
    use(this_lib)
    with _lib.KernelTimer() as kt:
        weighted()
        torch.cuda.synchronize()
    split = {k: {"ms": v[0], "launches": v[1]} for k, v in sorted(kt.stats.items(), key=lambda kv: -kv[1][0])}
    med = {k: float(np.median(v)) for k, v in ms.items()}
    ka, kb = "(a) forward + nll, this tree", "(b) forward_grad + weighted per_molecule_grad"
    print(f"{a.mols} x {a.atoms} atoms, {a.layers} layers, H {a.hid}, nf {a.nf}; ms per step, {a.windows} windows of "
          f"{a.iters}; losses {losses}")
    for k, v in ms.items():
        print(f"  {k:48s} " + "  ".join(f"{x:8.3f}" for x in v) + f"   median {med[k]:8.3f}  "
              f"min {min(v):8.3f}  max {max(v):8.3f}")
    print(f"(b) - (a), medians: {med[kb] - med[ka]:+.3f} ms")
    print("per-kernel split of one step (b) (event timer):")
    for k, v in split.items():
        print(f"  {k:36s} {v['ms']:8.3f} ms  {v['launches']:4d} launches")
    line = {"shape": {k: v for k, v in vars(a).items() if k not in ("out", "parent_lib")}, "losses": losses,
            "ms_per_step": ms, "median_ms": med, "b_minus_a_ms": med[kb] - med[ka], "kernel_split_b": split}
    print(json.dumps(line))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(line, fh, indent=1)


if __name__ == "__main__":
    main()
