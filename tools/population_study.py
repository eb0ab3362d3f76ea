#!/usr/bin/env python3
"""What population annealing buys and costs on one MI355X (profiles/population_annealing.md).

    python tools/population_study.py [--chains 65536] [--n-steps 100000] [--resample-every 1000] [--Ns 12 15] [--out FILE.json]

Board, random init, linear 1 -> 3, seeds 42 + r, no trace.  Per N:
1. plain annealing: one launch (mcq_run_device), wall time around launch + wait and the sweep kernel's own time (HIP events);
2. the same chains as device-resident segments of `resample_every` steps WITHOUT resampling (restore + sweep + checkpoint per segment);
3. population annealing with one population of all chains (population.anneal_population): min / p1 / p10 / median of best_energy against
   those of 1., the distinct parents of every boundary, wall time;
4. mcq_resample_device alone (plan + gather + fold) on the energies and placements a segment left, by HIP events."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def quantiles(best):
    import numpy as np

    return {"min": int(best.min()), "p1": float(np.percentile(best, 1)), "p10": float(np.percentile(best, 10)), "median": float(np.median(best)),
            "p90": float(np.percentile(best, 90)), "max": int(best.max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=65536)
    ap.add_argument("--n-steps", type=int, default=100000)
    ap.add_argument("--resample-every", type=int, default=1000)
    ap.add_argument("--Ns", type=int, nargs="+", default=[12, 15])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import ctypes

    import numpy as np
    import torch

    import mcq_amd

    abi, pop = mcq_amd.abi, mcq_amd.population
    sp = {"type": "linear_annealing", "beta_start": 1.0, "beta_end": 3.0}
    st = torch.cuda.current_stream()
    n, T, S = args.chains, args.n_steps, args.resample_every
    seeds = abi.seeds_for(42, n)
    K = -(-T // S)
    report = {"chains": n, "n_steps": T, "resample_every": S, "boundaries": K - 1, "cases": []}
    for N in args.Ns:
        case = {"N": N}
        # 1. plain annealing, one launch
        run = mcq_amd._lib.DeviceRun(abi.make_params(N, T, "random", sp, n, mcmc_type="board", trace=False), seeds, trace=False)
        wall = []
        for _ in range(args.reps):
            st.synchronize()
            t0 = time.perf_counter()
            run.launch(st)
            st.synchronize()
            wall.append(time.perf_counter() - t0)
        init_ms, sweep_ms = run.launch_timed(st)
        plain = run.results()
        case["plain"] = {"wall_ms": min(wall) * 1e3, "init_kernel_ms": init_ms, "sweep_kernel_ms": sweep_ms, "best_energy": quantiles(plain["best_energy"])}
        del run
        # 2. segments without resampling
        if T % S == 0:
            run = mcq_amd._lib.DeviceRun(abi.make_params(N, S, "random", sp, n, mcmc_type="board", trace=False), seeds, trace=False, schedule_steps=T)
            wall = []
            for _ in range(args.reps):
                state = ss = None
                st.synchronize()
                t0 = time.perf_counter()
                for i in range(K):
                    run.launch_from(i * S, state=state, stream_state=ss, stream=st)
                    ss = run.checkpoint(ss, stream=st)
                    state = run.t["final_state"]
                st.synchronize()
                wall.append(time.perf_counter() - t0)
            seg = run.results()
            case["segments_only"] = {"wall_ms": min(wall) * 1e3, "final_equals_plain": bool(np.array_equal(seg["final_state"], plain["final_state"]))}
            # 4. the resampling call alone, on what the last segment left
            sb = abi.state_bytes(N, abi.MODE_BOARD)
            dev = run.t["final_state"].device
            tab = torch.from_numpy(abi.resample_table(2.0 * S / (T - 1)).view(np.int32)).to(dev)
            x = torch.from_numpy(np.array([0x9E3779B9], dtype=np.uint32).view(np.int32)).to(dev)
            out = torch.empty_like(run.t["final_state"])
            parent = torch.empty(n, dtype=torch.int32, device=dev)
            stats = torch.empty((1, 3), dtype=torch.int64, device=dev)
            acc = {k: torch.zeros_like(run.t[k]) for k in ("best_energy", "steps_to_best", "n_accepted", "near_ties", "stream_words", "best_state")}
            r = abi.Resample()
            r.n_chains, r.population, r.state_bytes, r.first_step = n, n, sb, S
            r.table, r.table_len, r.offsets, r.energies = tab.data_ptr(), tab.numel(), x.data_ptr(), run.t["final_energy"].data_ptr()
            r.state_in, r.state_out, r.parent, r.stats = run.t["final_state"].data_ptr(), out.data_ptr(), parent.data_ptr(), stats.data_ptr()
            for f in acc:
                setattr(r, "seg_" + f, run.t[f].data_ptr()), setattr(r, "run_" + f, acc[f].data_ptr())
            scratch = torch.empty(int(mcq_amd._lib.lib().mcq_resample_scratch_bytes(ctypes.byref(r))), dtype=torch.uint8, device=dev)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ms = []
            for _ in range(5):
                e0.record(st)
                mcq_amd._lib.resample_device(r, scratch, st)
                e1.record(st)
                st.synchronize()
                ms.append(e0.elapsed_time(e1))
            case["resample_call_ms"] = min(ms)
            del run
        # 3. population annealing
        wall, res, lin = [], None, None
        for _ in range(args.reps):
            tm = {}
            res, lin = pop.anneal_population(N, T, "random", sp, seeds, S, mcmc_type="board", trace=False, timings=tm)
            wall.append(tm["run_seconds"])
        dp = lin["distinct_parents"][:, 0]
        case["population"] = {"wall_ms": min(wall) * 1e3, "best_energy": quantiles(res["best_energy"]), "distinct_parents": [int(v) for v in dp],
                              "distinct_ancestors": int(len(np.unique(lin["ancestors"]))), "near_ties": int(res["near_ties"].sum())}
        case["per_boundary_ms"] = (case["population"]["wall_ms"] - case["plain"]["wall_ms"]) / max(1, K - 1)
        report["cases"].append(case)
        print(json.dumps(case), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
