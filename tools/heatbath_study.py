#!/usr/bin/env python3
"""Heat-bath column sweeps next to the Metropolis sweep at equal time and at fixed sweep counts, on one MI355X (profiles/heatbath.md).

    python tools/heatbath_study.py [--chains 65536] [--n-steps 100000] [--Ns 12 15] [--sweeps 700 445] [--form lines|counters] [--out FILE.json]
    python tools/heatbath_study.py --ab 8 12 15 16 [--chains 65536] [--out FILE.json]        (profiles/heatbath_counters.md)

Board, random init, linear 1 -> 3, seeds 42 + r, no trace.  Per N, in one process:
  (a) the Metropolis sweep at --n-steps steps: the sweep kernel's time by HIP events, min / p10 / median best_energy;
  -   the time of one heat-bath sweep (HIP events around one mcq_heatbath_device call of --probe sweeps, best of --reps after a warm-up)
      next to one walk of the quench kernel (a call with max_passes = 1 and no conflict map is two walks);
  (b) heat-bath at the sweep count whose time, by that figure, is the closest below (a)'s;
  (c) heat-bath at the given sweep count, plain and with resample_every such that there are about 100 boundaries.
For every heat-bath run: min / p10 / median best_energy, the kernel's time by HIP events (plain) or the wall time of the whole chain of
launches (resampled), ms per sweep, column updates per second, the share of updates that changed a height.
--form is the kernel of every heat-bath run (heatbath.FORMS; the results do not depend on it, the times do).
--ab is the timing leg alone, for both forms in one process: per N, --chains random boards, --probe sweeps 1 -> 3, the best of --reps
calls by HIP events after a warm-up, the forms alternated (lines, counters, lines, counters); the sums of energy_out and n_changed of
the two forms must be equal.  The spread between the two rounds of one form is the noise of the figure."""
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
    ap.add_argument("--n-steps", type=int, default=100000)
    ap.add_argument("--Ns", type=int, nargs="+", default=[12, 15])
    ap.add_argument("--sweeps", type=int, nargs="+", default=[700, 445])
    ap.add_argument("--probe", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--form", choices=("lines", "counters"), default="lines")
    ap.add_argument("--ab", type=int, nargs="+", default=None, metavar="N")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    import mcq_amd

    abi, hb = mcq_amd.abi, mcq_amd.heatbath
    if mcq_amd._lib.device_count() < 1:
        raise RuntimeError("heatbath_study needs a GPU")
    sp = {"type": "linear_annealing", "beta_start": 1.0, "beta_end": 3.0}
    st = torch.cuda.current_stream()
    dev = torch.device("cuda", torch.cuda.current_device())
    n, T = args.chains, args.n_steps
    seeds = abi.seeds_for(42, n)
    dseeds = torch.from_numpy(seeds.view(np.int32).copy()).to(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    report = {"chains": n, "n_steps": T, "device": torch.cuda.get_device_name(dev), "cases": []}

    def timed(fn):
        e0.record(st)
        out = fn()
        e1.record(st)
        st.synchronize()
        return out, e0.elapsed_time(e1)

    def save():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(report, f, indent=1)

    if args.ab is not None:
        from tests import quench_util as qu

        report["ab"] = []
        betas = abi.beta_values(sp, args.probe)
        for N in args.ab:
            start = torch.from_numpy(qu.random_boards(N, n, N)).to(dev)
            tab = hb.device_table(betas, dev)
            case = {"N": N, "sweeps": args.probe, "lines_ms_per_sweep": [], "counters_ms_per_sweep": []}
            sums = {}
            for rnd in range(2):
                for form in hb.FORMS:
                    hb.heatbath_device(N, start, dseeds, tab[:2], stream=st, form=form)  # warm-up
                    st.synchronize()
                    runs = [timed(lambda: hb.heatbath_device(N, start, dseeds, tab, stream=st, form=form)) for _ in range(args.reps)]
                    case[form + "_ms_per_sweep"].append(min(ms for _, ms in runs) / args.probe)
                    res = runs[-1][0]
                    sums.setdefault(form, []).append((int(res["energy_out"].sum().item()), int(res["n_changed"].sum().item())))
            assert len(set(sums["lines"] + sums["counters"])) == 1, f"N={N}: the two forms disagree: {sums}"
            case["energy_out_sum"], case["n_changed_sum"] = sums["lines"][0]
            lo, co = case["lines_ms_per_sweep"], case["counters_ms_per_sweep"]
            case["change"] = min(co) / min(lo) - 1.0
            case["spread"] = max(max(lo) / min(lo), max(co) / min(co)) - 1.0
            report["ab"].append(case)
            print(json.dumps(case), flush=True)
        save()
        return

    report["form"] = args.form
    for N, fixed in zip(args.Ns, args.sweeps):
        Q = N * N
        case = {"N": N}
        run = mcq_amd._lib.DeviceRun(abi.make_params(N, T, "random", sp, n, mcmc_type="board", trace=False), seeds, trace=False)
        run.launch(st)
        st.synchronize()
        init_ms, sweep_ms = run.launch_timed(st)
        plain = run.results()
        case["metropolis"] = {"steps": T, "sweep_kernel_ms": sweep_ms, "init_kernel_ms": init_ms, "best_energy": quantiles(plain["best_energy"]),
                              "accepted_share": float(plain["n_accepted"].sum() / (n * T))}
        del run
        first, _ = mcq_amd.experiments.start_chains(N, 0, "random", sp, seeds, mcmc_type="board", trace=False, states=True)
        start = torch.from_numpy(np.ascontiguousarray(first["final_state"])).to(dev)

        def kernel(n_sweeps):
            """one mcq_heatbath_device call of n_sweeps sweeps of the schedule stretched over them; (results, ms by HIP events)"""
            tab = hb.device_table(abi.beta_values(sp, n_sweeps), dev)
            st.synchronize()
            return timed(lambda: hb.heatbath_device(N, start, dseeds, tab, stream=st, form=args.form))

        kernel(2)  # warm-up: loads the code object
        probe = [kernel(args.probe)[1] / args.probe for _ in range(args.reps)]
        minima = mcq_amd.quench.quench_device(N, start, conflicts=False, stream=st)["state"]
        mcq_amd.quench.quench_device(N, minima, max_passes=1, conflicts=False, stream=st)
        walks = [timed(lambda: mcq_amd.quench.quench_device(N, minima, max_passes=1, conflicts=False, stream=st))[1] / 2 for _ in range(args.reps)]
        case["one_sweep_ms"] = {"heatbath": min(probe), "heatbath_all": probe, "quench_walk": min(walks), "quench_walk_all": walks, "probe_sweeps": args.probe}

        def describe(res, n_sweeps, ms, what):
            best = res["best_energy"].cpu().numpy() if hasattr(res["best_energy"], "cpu") else res["best_energy"]
            changed = res["n_changed"].cpu().numpy() if hasattr(res["n_changed"], "cpu") else res["n_changed"]
            return {"sweeps": n_sweeps, "column_updates_per_chain": n_sweeps * Q, what: ms, "ms_per_sweep": ms / n_sweeps,
                    "column_updates_per_second": n * n_sweeps * Q / (ms * 1e-3), "changed_share": float(changed.sum() / (n * n_sweeps * Q)),
                    "best_energy": quantiles(best)}

        equal = max(1, int(sweep_ms / min(probe)))
        res, ms = kernel(equal)
        while ms >= sweep_ms and equal > 1:  # the closest BELOW the Metropolis sweep's time, as measured
            equal -= max(1, int(np.ceil((ms - sweep_ms) / (ms / equal))))
            res, ms = kernel(equal)
        case["equal_time"] = describe(res, equal, ms, "kernel_ms")
        res, ms = kernel(fixed)
        case["fixed_plain"] = describe(res, fixed, ms, "kernel_ms")
        S = max(1, fixed // 100)
        hb.anneal_heatbath(N, fixed, first["final_state"], sp, seeds, resample_every=S, form=args.form)  # warm-up
        t0 = time.perf_counter()
        res, lin = hb.anneal_heatbath(N, fixed, first["final_state"], sp, seeds, resample_every=S, form=args.form)
        wall = (time.perf_counter() - t0) * 1e3
        case["fixed_resampled"] = dict(describe(res, fixed, wall, "wall_ms"), resample_every=S, boundaries=len(lin["lengths"]) - 1,
                                       distinct_parents_mean=float(lin["distinct_parents"].mean()))
        t0 = time.perf_counter()
        res = hb.anneal_heatbath(N, fixed, first["final_state"], sp, seeds, form=args.form)
        case["fixed_plain"]["wall_ms_anneal_heatbath"] = (time.perf_counter() - t0) * 1e3
        report["cases"].append(case)
        print(json.dumps(case), flush=True)
    save()


if __name__ == "__main__":
    main()
