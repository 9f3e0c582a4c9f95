"""Timing of the prepared edge list (enflow_amd.data.EdgeList) for DESIGN.md 3h:
the 1024 x 22-atom batch with its own Edges.reference() list (372 687 edges),
H = 128, nf = 5.  Host clock around a final synchronise, three windows per path,
alternating, after warm-up; the baseline is the plain-list path in this process.

  (a) net(h, list) against net(h, prepared)                      200 calls per window
  (b) forward_edges + backward, plain list against prepared       50 calls per window
  (c) the one-off build: EdgeList (CSR) and its CSC, against torch's
      EGCL._list_csr / _list_csc on the same list                200 calls per window
  (d) net(h, d.edges), the handle path, for scale                 200 calls per window

then 20 calls of each prepared path under the library's event timer (kernel ms
per launch).  For the GPU box:

    python tools/edge_list_handle_timing.py [OUT.json]   (default: edge_list_handle_timing.json)"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from enflow_amd import _lib                                   # noqa: E402
from enflow_amd.data import Data, EdgeList                    # noqa: E402
from enflow_amd.data.synthetic import make_molecules          # noqa: E402
from enflow_amd.nn import EGCL                                # noqa: E402

DEV = "cuda:0"
WINDOWS = 3


class List:
    def __init__(self, row, col, coord_diff):
        self.row, self.col, self.coord_diff = row, col, coord_diff


def window(fn, calls):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / calls * 1e3


def alternate(paths, calls, warm=10):
    """{name: [ms per call, one per window]}: the paths in turn, WINDOWS times."""
    for fn in paths.values():
        for _ in range(warm):
            fn()
    out = {k: [] for k in paths}
    for _ in range(WINDOWS):
        for k, fn in paths.items():
            out[k].append(window(fn, calls))
    return out


def kernels(fn, calls=20):
    with _lib.KernelTimer() as t:
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
    return {k: v[0] / calls for k, v in t.stats.items()}   # ms per call, every launch of the kernel in it


def main():
    d = Data.from_arrays(make_molecules(1024, 22, nf=5, seed=1000), device=DEV)
    ref = d.edges.reference()
    row, col, cd = ref.row, ref.col, ref.coord_diff
    n, E = int(d.h.shape[0]), int(row.numel())
    torch.manual_seed(0)
    net = EGCL(5, 5, 128).to(DEV)
    h = d.h
    plain = List(row, col, cd)
    prepared = EdgeList(row, col, cd, num_nodes=n)
    g = torch.Generator(DEV).manual_seed(1)
    w = [torch.randn(s, device=DEV, generator=g) for s in ((n, 1), (n, 3), (n, 5))]
    out = {"device": torch.cuda.get_device_name(0), "nodes": n, "edges": E, "hidden_nf": 128, "node_nf": 5,
           "windows": WINDOWS}

    def fwd(edges):
        def call():
            with torch.no_grad():
                net(h, edges)
        return call

    def fwd_bwd(make):
        def call():
            net.zero_grad(set_to_none=True)
            ht = h.detach().requires_grad_(True)
            lst = make(cd.detach().requires_grad_(True))
            outs = net.forward_edges(ht, lst)
            sum((x * o).sum() for x, o in zip(w, outs)).backward()
        return call

    # (a) + (d)
    out["forward_ms"] = alternate({"list": fwd(plain), "prepared": fwd(prepared), "data_edges_handle": fwd(d.edges)}, 200)
    # (b)
    out["forward_backward_ms"] = alternate({"list": fwd_bwd(lambda c: List(row, col, c)),
                                            "prepared": fwd_bwd(prepared.with_coord_diff)}, 50)

    # (c) the one-off builds; a fresh topology per call (the CSC timed as CSR + CSC minus CSR)
    def hip_csr():
        EdgeList(row, col, cd, num_nodes=n)

    def hip_csr_csc():
        EdgeList(row, col, cd, num_nodes=n).topology.csc()

    colp = prepared.topology.csr()[1]
    b = alternate({"hip_csr": hip_csr, "hip_csr_and_csc": hip_csr_csc,
                   "torch_list_csr": lambda: EGCL._list_csr(n, row, col, cd),
                   "torch_list_csc": lambda: EGCL._list_csc(n, colp)}, 200)
    b["hip_csc"] = [both - one for both, one in zip(b["hip_csr_and_csc"], b["hip_csr"])]
    out["build_ms"] = b
    out["kernel_ms_per_call"] = {"forward_prepared": kernels(fwd(prepared)),
                                 "forward_backward_prepared": kernels(fwd_bwd(prepared.with_coord_diff)),
                                 "build_csr_and_csc": kernels(hip_csr_csc)}
    f, fb = out["forward_ms"], out["forward_backward_ms"]
    out["prepared_faster_in_every_window"] = {
        "forward": all(p < q for p, q in zip(f["prepared"], f["list"])),
        "forward_backward": all(p < q for p, q in zip(fb["prepared"], fb["list"])),
        "csr_build": all(p < q for p, q in zip(b["hip_csr"], b["torch_list_csr"])),
        "csc_build": all(p < q for p, q in zip(b["hip_csc"], b["torch_list_csc"]))}
    out["median_ms"] = {k: {p: float(np.median(v)) for p, v in out[k].items()}
                        for k in ("forward_ms", "forward_backward_ms", "build_ms")}
    print(json.dumps(out, indent=1))
    with open(sys.argv[1] if len(sys.argv) > 1 else "edge_list_handle_timing.json", "w") as fh:
        json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
