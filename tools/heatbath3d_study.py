#!/usr/bin/env python3
"""Heat-bath queen sweeps of full_3d placements next to the Metropolis sweep at equal time and at five times that time, and next to
one pass of the full_3d quench over the same placements, on one MI355X (profiles/heatbath3d.md).

    python tools/heatbath3d_study.py [--chains 65536] [--N 12] [--n-steps 100000] [--metropolis-ms MS] [--larger 24:1024] [--out FILE.json]

full_3d, Q = N^2, random init, seeds 42 + r, no trace.  In one process:
  (a) the Metropolis sweep of bench.py --config c3 (exponential 1 -> 3, --n-steps steps): the sweep kernel's time by HIP events and
      min / p10 / median best_energy.  --metropolis-ms replaces the time by the figure bench.py --config c3 printed in the same session
      (kernel_ms.sweep); the in-process figure is recorded next to it.
  -   the time of one heat-bath sweep (HIP events around one mcq_heatbath3d_device call of --probe sweeps, best of --reps after a
      warm-up) next to one pass of quench_queens_device (max_passes = 1, no conflict map) over the same placements: the two kernels
      share the field traffic.  The same two figures for every --larger N:chains.
  (b) heat-bath, linear 1 -> 3, at the sweep count whose time, by that figure, is the closest below (a)'s;
  (c) heat-bath, linear 1 -> 3, at five times that count, plain and with resample_every such that there are about 100 boundaries.
For every heat-bath run: min / p10 / median best_energy, the kernel's time by HIP events (plain) or the wall time of the whole chain of
launches (resampled), ms per sweep, queen updates per second, the share of updates that changed a cell."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def quantiles(e):
    import numpy as np

    return {"min": int(e.min()), "p10": float(np.percentile(e, 10)), "median": float(np.median(e)), "mean": float(e.mean()), "max": int(e.max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=65536)
    ap.add_argument("--N", type=int, default=12)
    ap.add_argument("--n-steps", type=int, default=100000)
    ap.add_argument("--metropolis-ms", type=float, default=None, help="kernel_ms.sweep of bench.py --config c3 from the same session")
    ap.add_argument("--larger", nargs="*", default=["24:1024"], help="N:chains of further cubes: ms per sweep and the quench pass only")
    ap.add_argument("--factor", type=int, default=5)
    ap.add_argument("--probe", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    import mcq_amd

    abi, hb, quench = mcq_amd.abi, mcq_amd.heatbath, mcq_amd.quench
    if mcq_amd._lib.device_count() < 1:
        raise RuntimeError("heatbath3d_study needs a GPU")
    lin = {"type": "linear_annealing", "beta_start": 1.0, "beta_end": 3.0}
    exp = {"type": "exponential_annealing", "beta_start": 1.0, "beta_end": 3.0}
    st = torch.cuda.current_stream()
    dev = torch.device("cuda", torch.cuda.current_device())
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    report = {"device": torch.cuda.get_device_name(dev), "cases": []}

    def timed(fn):
        e0.record(st)
        out = fn()
        e1.record(st)
        st.synchronize()
        return out, e0.elapsed_time(e1)

    def placements(N, n):
        seeds = abi.seeds_for(42, n)
        first, _ = mcq_amd.experiments.start_chains(N, 0, "random", lin, seeds, mcmc_type="full_3d", trace=False, states=True)
        host = np.ascontiguousarray(first["final_state"], dtype=np.uint8).reshape(n, -1)
        return seeds, host, torch.from_numpy(host).to(dev), torch.from_numpy(seeds.view(np.int32).copy()).to(dev)

    def one_sweep(N, start, dseeds):
        """ms of one heat-bath sweep at beta = 1 .. 3 and of one quench pass over the same placements"""
        def kernel(k):
            tab = hb.device_table(abi.beta_values(lin, k), dev)
            st.synchronize()
            return timed(lambda: hb.heatbath_queens_device(N, start, dseeds, tab, best_state=False, stream=st))[1]

        kernel(1)  # warm-up: loads the code object
        probe = [kernel(args.probe) / args.probe for _ in range(args.reps)]
        quench.quench_queens_device(N, start, max_passes=1, conflicts=False, stream=st)
        st.synchronize()
        passes = [timed(lambda: quench.quench_queens_device(N, start, max_passes=1, conflicts=False, stream=st))[1] for _ in range(args.reps)]
        return {"heatbath": min(probe), "heatbath_all": probe, "quench_pass": min(passes), "quench_pass_all": passes, "probe_sweeps": args.probe,
                "heatbath_over_quench_pass": min(probe) / min(passes)}

    N, n, T = args.N, args.chains, args.n_steps
    Q = N * N
    seeds, host, start, dseeds = placements(N, n)
    case = {"N": N, "Q": Q, "chains": n}
    run = mcq_amd._lib.DeviceRun(abi.make_params(N, T, "random", exp, n, mcmc_type="full_3d", trace=False), seeds, trace=False)
    run.launch(st)
    st.synchronize()
    init_ms, sweep_ms = run.launch_timed(st)
    plain = run.results()
    case["metropolis"] = {"steps": T, "schedule": exp, "sweep_kernel_ms": sweep_ms, "init_kernel_ms": init_ms, "bench_c3_sweep_kernel_ms": args.metropolis_ms,
                          "best_energy": quantiles(plain["best_energy"]), "accepted_share": float(plain["n_accepted"].sum() / (n * T))}
    del run
    budget = sweep_ms if args.metropolis_ms is None else args.metropolis_ms
    case["one_sweep_ms"] = one_sweep(N, start, dseeds)
    per = case["one_sweep_ms"]["heatbath"]

    def kernel(n_sweeps):
        tab = hb.device_table(abi.beta_values(lin, n_sweeps), dev)
        st.synchronize()
        return timed(lambda: hb.heatbath_queens_device(N, start, dseeds, tab, stream=st))

    def describe(res, n_sweeps, ms, what):
        best = res["best_energy"].cpu().numpy() if hasattr(res["best_energy"], "cpu") else res["best_energy"]
        changed = res["n_changed"].cpu().numpy() if hasattr(res["n_changed"], "cpu") else res["n_changed"]
        return {"sweeps": n_sweeps, "queen_updates_per_chain": n_sweeps * Q, what: ms, "ms_per_sweep": ms / n_sweeps,
                "queen_updates_per_second": n * n_sweeps * Q / (ms * 1e-3), "changed_share": float(changed.sum() / (n * n_sweeps * Q)),
                "best_energy": quantiles(best), "zero_energy_chains": int((best == 0).sum())}

    equal = max(1, int(budget / per))
    res, ms = kernel(equal)
    while ms >= budget and equal > 1:  # the closest BELOW the Metropolis sweep's time, as measured
        equal -= max(1, int(np.ceil((ms - budget) / (ms / equal))))
        res, ms = kernel(equal)
    case["equal_time"] = dict(describe(res, equal, ms, "kernel_ms"), budget_ms=budget)
    print(json.dumps({"equal_time": case["equal_time"]}), flush=True)
    more = args.factor * equal
    res, ms = kernel(more)
    case["more_time_plain"] = dict(describe(res, more, ms, "kernel_ms"), factor=args.factor)
    print(json.dumps({"more_time_plain": case["more_time_plain"]}), flush=True)
    S = max(1, more // 100)
    R = min(n, 1 << 19)
    hb.anneal_heatbath(N, 2 * S, host, lin, seeds, resample_every=S, population=R, mcmc_type="full_3d")  # warm-up
    t0 = time.perf_counter()
    res, lineage = hb.anneal_heatbath(N, more, host, lin, seeds, resample_every=S, population=R, mcmc_type="full_3d")
    wall = (time.perf_counter() - t0) * 1e3
    case["more_time_resampled"] = dict(describe(res, more, wall, "wall_ms"), factor=args.factor, resample_every=S, population=R,
                                       boundaries=len(lineage["lengths"]) - 1, distinct_parents_mean=float(lineage["distinct_parents"].mean()))
    report["cases"].append(case)
    print(json.dumps(case), flush=True)

    for shape in args.larger:
        N2, n2 = (int(x) for x in shape.split(":"))
        _, _, start2, dseeds2 = placements(N2, n2)
        other = {"N": N2, "Q": N2 * N2, "chains": n2, "one_sweep_ms": one_sweep(N2, start2, dseeds2)}
        report["cases"].append(other)
        print(json.dumps(other), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
