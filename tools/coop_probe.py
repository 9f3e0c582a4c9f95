"""Cooperative leftover tiles (enflow_set_coop_tiles): interleaved A/B of
bench.py's flow step in ONE process, as tools/order_probe.py.

    python tools/coop_probe.py [--mode forward|generate|chain] [--parent PARENT.so [PARENT_COPY.so]]
                               [--rounds 6] [--steps 40] [--out FILE.json]

Configurations, run round-robin `rounds` times forward and then in reverse
order: a build of the parent commit (twice when a second copy of the file is
given: the parent-against-parent spread of the session), this build with the
switch off (coop0) and on (coop1).  Per configuration and round: the step time
from one event pair around `steps` back-to-back steps, then the flow kernel's
time by the library's own event pairs (KernelTimer).  Outputs: bitwise against
the first configuration, and each array's normwise difference from it."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="forward")
    ap.add_argument("--parent", nargs="*", default=[])
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import bench
    from enflow_amd import _lib
    from enflow_amd.data.synthetic import make_molecules
    dev = torch.device("cuda", 0)
    c = bench.MODES[args.mode]
    model = bench.build_model(dev, c["layers"])
    model.gemm_precision = c["prec"]
    inp = bench.batch_tensors(make_molecules(c["mols"], c["atoms"], nf=bench.NF, seed=1000, chain=c["chain"]), dev)
    gen = torch.Generator(device="cpu").manual_seed(0)
    new_lib = _lib.LIB_PATH
    cfgs = [(f"parent{i + 1}", p, None) for i, p in enumerate(args.parent)]
    cfgs += [("coop0", new_lib, 0), ("coop1", new_lib, 1)]

    def select(path, on):
        _lib._libs.clear()
        _lib.LIB_PATH = os.path.abspath(path)
        model._layers_key = None
        model.dequantize._packed_key = None
        if on is not None:
            _lib.set_coop_tiles(on)

    runners, outs = {}, {}
    for name, path, on in cfgs:
        select(path, on)
        runners[name] = bench.FlowRunner(model, inp, c["atoms"], c["reverse"], dev, gen)

    def steps(name, n):
        r = runners[name]
        r.calls = 0
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            r.step()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    kname = "lf_flow_kernel<rev>" if c["reverse"] else "lf_flow_kernel<fwd>"
    res = {name: {"step_ms": [], "kernel_ms": []} for name, _, _ in cfgs}
    for name, path, on in cfgs:      # pack, warm, clocks up
        select(path, on)
        steps(name, 200)
    seq = []
    for rnd in range(args.rounds):
        seq += [cfgs, cfgs[::-1]][rnd % 2]
    for name, path, on in seq:
        select(path, on)
        steps(name, 10)
        res[name]["step_ms"].append(steps(name, args.steps))
        with _lib.KernelTimer() as t:
            for _ in range(10):
                runners[name].step()
        res[name]["kernel_ms"].append(t.ms_per_launch(kname) if kname in t.stats else float("nan"))
        runners[name].calls = 0
        runners[name].step()
        runners[name].check()
        outs[name] = runners[name].outputs()
    first = cfgs[0][0]
    report = {"workload": bench.workload_name(args.mode), "rounds": args.rounds, "steps_per_round": args.steps,
              "device": torch.cuda.get_device_name(0), "configs": {}}
    for name, _, _ in cfgs:
        r = res[name]
        same = all(torch.equal(outs[name][k], outs[first][k]) for k in outs[first])
        nw = {k: float((outs[name][k].double() - outs[first][k].double()).norm() /
                       outs[first][k].double().norm().clamp_min(1e-300)) for k in outs[first]}
        report["configs"][name] = {
            "step_ms_rounds": [round(x, 5) for x in r["step_ms"]], "step_ms_median": statistics.median(r["step_ms"]),
            "kernel_ms_rounds": [round(x, 5) for x in r["kernel_ms"]],
            "kernel_ms_median": statistics.median(r["kernel_ms"]),
            "outputs_bitwise_equal_to_" + first: same, "normwise_difference_from_" + first: nw}
        print(f"{name:8s} step {statistics.median(r['step_ms']):.4f} ms  {kname} "
              f"{statistics.median(r['kernel_ms']):.4f} ms  bitwise = {first}: {same}  normwise "
              f"{ {k: f'{v:.1e}' for k, v in nw.items()} }", flush=True)
    names = [n for n, _, _ in cfgs]
    for a, b in [(x, y) for i, x in enumerate(names) for y in names[i + 1:]]:
        for what in ("step_ms", "kernel_ms"):
            d = [(y - x) / x * 100 for x, y in zip(res[a][what], res[b][what])]
            report.setdefault("pairwise_percent", {})[f"{b}_vs_{a}_{what}"] = [round(v, 3) for v in d]
            print(f"{b} vs {a} {what}: per round {[round(v, 2) for v in d]} %  median {statistics.median(d):+.2f} %")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(report, fh, indent=1)


if __name__ == "__main__":
    main()
