"""Measurements for DESIGN.md: one edge_index materialisation next to today's
Edges.row / col, for the 1024 x 22 bench batch and one 2944-atom LJ box; the
worst coord_diff error against the goldens.

    python profiles/measure_edge_list.py [OUT.json]    (default: edge_list_measure.json)"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from enflow_amd import _lib                                              # noqa: E402
from enflow_amd.data import Data                                         # noqa: E402
from enflow_amd.data.synthetic import make_molecules, make_lj_systems   # noqa: E402
from _fixtures import load, data_from_fixture                            # noqa: E402

DEV = "cuda:0"
out = {"device": torch.cuda.get_device_name(0)}


def new_order(d):
    e = d.edges
    return e.edge_index


def shipped(d):
    e = d.edges
    return e.row, e.col


def timed(fn, d, n):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(n):
        fn(d)
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / n * 1e3


def measure(name, b, reps):
    d = Data.from_arrays(b, device=DEV)
    for _ in range(5):   # warm-up of both
        new_order(d), shipped(d)
    a, s = [], []
    for _ in range(5):   # alternate the two, 5 windows each
        a.append(timed(new_order, d, reps))
        s.append(timed(shipped, d, reps))
    E = int(new_order(d).shape[1])
    with _lib.KernelTimer() as t:
        for _ in range(10):
            new_order(d)
        torch.cuda.synchronize()
    kern = {k: v[0] / v[1] for k, v in t.stats.items()}
    out[name] = dict(edges=E, atoms=int(d.pos.shape[0]), reps_per_window=reps,
                     edge_index_ms=dict(median=float(np.median(a)), min=min(a), max=max(a)),
                     row_col_ms=dict(median=float(np.median(s)), min=min(s), max=max(s)),
                     kernel_ms_per_launch=kern)
    print(name, json.dumps(out[name]), flush=True)


worst = {}
for g in ("edges_box20", "edges_box5", "edges_extent"):
    inp, ref = load(g)
    cd = data_from_fixture(inp, DEV).edges.reference().coord_diff.cpu().numpy()
    worst[g] = float(np.max(np.abs(cd - ref["coord_diff"].reshape(-1, 3))))
out["golden_coord_diff_worst_abs_err"] = worst
print("goldens", worst, flush=True)

measure("bench_1024x22", make_molecules(1024, 22, nf=5, seed=1000), 2000)
lj = make_lj_systems([2944], seed=3000, nf=5)
lj["pos"] = lj["pos"] - np.round(lj["pos"] / lj["box"]) * lj["box"]
measure("lj_box_2944", lj, 1000)

with open(sys.argv[1] if len(sys.argv) > 1 else "edge_list_measure.json", "w") as fh:
    json.dump(out, fh, indent=1)
print("done")
