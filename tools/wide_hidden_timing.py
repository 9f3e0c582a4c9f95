"""Time the flow at hidden_nf 256 (the wide layer kernel, csrc/enflow_wide.hip)
against the same batch at hidden_nf 128 forced onto the large-system path
(ENFLOW_LARGE_MIN_ATOMS=1), forward and reverse, so that like is compared with
like: the same launch sequence, only the layer kernel differs.  --prec picks
the GEMM precision of both models (f16x3, the default, or f32).  One process, alternating
windows, device events around each window, one synchronise at the end.

    python tools/wide_hidden_timing.py [--mols 1024] [--atoms 22] [--layers 8] [--prec f16x3] [--out FILE.json]

Prints a table and one JSON line; needs the GPU.  Numbers for DESIGN.md only (no bars).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK = {"f32": 157.3e12, "f16x3": 2516.6e12}      # MI355X fp32 / dense fp16 matrix peak, FLOP/s
ISSUED = {"f32": 1, "f16x3": 3}                    # MFMA products issued per useful multiply-add


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mols", type=int, default=1024)
    ap.add_argument("--atoms", type=int, default=22)
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--nf", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--prec", default="f16x3", choices=sorted(PEAK))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    os.environ["ENFLOW_LARGE_MIN_ATOMS"] = "1"      # read per call: H 128 takes the large path too
    from enflow_amd import _lib
    from enflow_amd.nn import EGCL, ArgMax
    from enflow_amd.flow import LFIntegrator
    from enflow_amd.data import Data
    from enflow_amd.data.synthetic import make_molecules, default_dt
    dev = "cuda:0"
    b = make_molecules(a.mols, a.atoms, nf=a.nf, seed=1)
    data = Data.from_arrays(b, device=dev)
    noise = torch.randn_like(data.h)
    models = {}
    for hid in (128, 256):
        torch.manual_seed(0)
        m = LFIntegrator([EGCL(a.nf, a.nf, hid) for _ in range(a.layers)], ArgMax(a.nf, hid), dt=default_dt()).to(dev)
        m.gemm_precision = a.prec
        models[hid] = m
    outs = {}

    def fwd(hid):
        with torch.no_grad():
            outs[hid] = models[hid](data.clone(), noise=noise)[0]

    def rev(hid):
        with torch.no_grad():
            models[hid].reverse(outs[hid].clone())

    paths = {f"{k} H{hid}": (lambda f=f, hid=hid: f(hid)) for hid in (128, 256) for k, f in (("forward", fwd), ("reverse", rev))}
    for f in paths.values():
        for _ in range(2):
            f()
    torch.cuda.synchronize()
    ev = {k: [] for k in paths}
    for _ in range(a.windows):
        for k, f in paths.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                f()
            e1.record()
            ev[k].append((e0, e1))
    torch.cuda.synchronize()
    ms = {k: [e0.elapsed_time(e1) / a.iters for e0, e1 in v] for k, v in ev.items()}
    med = {k: float(np.median(v)) for k, v in ms.items()}
    split = {}
    for hid in (128, 256):
        with _lib.KernelTimer() as kt:
            fwd(hid)
            torch.cuda.synchronize()
        split[hid] = {k: {"ms": v[0], "launches": v[1]} for k, v in kt.stats.items()}
    # useful GEMM work of one layer from the input geometry's unique pairs (layer 0's list;
    # later layers' lists differ a little): edge_nn.0, edge_nn.2, coord_nn.0 per pair, node_nn /
    # vel_scaling_nn per atom; 2 FLOP per multiply-add
    e = data.edges
    n_at = int(data.h.shape[0])
    pairs = int(torch.unique(e.row.to(torch.int64) * n_at + e.col.to(torch.int64)).numel())
    flop, frac = {}, {}
    for hid, name in ((128, "lg_layer_kernel"), (256, "lg_wide_layer_kernel")):
        per_pair = 2 * ((2 * a.nf + 1) * hid + 2 * hid * hid)
        per_atom = 2 * ((hid + a.nf) * hid + a.nf * hid + a.nf * hid)
        flop[hid] = pairs * per_pair + n_at * per_atom
        k = split[hid].get(name)
        if k:
            frac[hid] = ISSUED[a.prec] * flop[hid] / (k["ms"] / k["launches"] * 1e-3) / PEAK[a.prec]
    print(f"{a.mols} x {a.atoms} atoms, {a.layers} layers, nf {a.nf}, {a.prec} GEMMs, large-system path; ms per call, "
          f"{a.windows} windows of {a.iters}; {pairs} unique pairs")
    for k, v in ms.items():
        print(f"  {k:14s} " + "  ".join(f"{x:8.3f}" for x in v) + f"   median {med[k]:8.3f}")
    ratio = {d: med[f"{d} H256"] / med[f"{d} H128"] for d in ("forward", "reverse")}
    print("H256 / H128:", ratio, f" issued-FLOP fraction of the {a.prec} pipe, layer kernel:", frac)
    for hid in (128, 256):
        for k, v in sorted(split[hid].items(), key=lambda kv: -kv[1]["ms"]):
            print(f"  H{hid} {k:28s} {v['ms']:8.3f} ms  {v['launches']:4d} launches")
    line = {"shape": {k: v for k, v in vars(a).items() if k != "out"}, "ms_per_call": ms, "median_ms": med,
            "ratio_h256_over_h128": ratio, "unique_pairs_layer0": pairs, "useful_gemm_flop_per_layer": flop,
            "issued_flop_fraction_of_pipe": frac, "kernel_split_forward": split}
    print(json.dumps(line))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(line, fh, indent=1)


if __name__ == "__main__":
    main()
