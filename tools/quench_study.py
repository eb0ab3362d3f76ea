#!/usr/bin/env python3
"""What the quench finds below the placements annealing hands back, and what it costs, on one MI355X (profiles/quench.md).

    python tools/quench_study.py [--chains 65536] [--n-steps 100000] [--resample-every 1000] [--Ns 12 15] [--out FILE.json]

Board, random init, linear 1 -> 3, seeds 42 + r, no trace: the shapes of profiles/population_annealing.md.  Per N, for plain annealing
(one launch) and for population annealing (one population of all chains), and for best_state and final_state of each:
  - min / p10 / median energy before and after the quench (energy_in is the device recount: it is compared with the sweep's own figure);
  - the share of placements that were local minima already (n_moves == 0), moves and passes per chain;
  - the quench kernel's time by HIP events (best of --reps, after a warm-up call), next to the sweep kernel's time (plain) or the wall
    time of the whole chain of launches (population) from the same process."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def quantiles(e):
    import numpy as np

    return {"min": int(e.min()), "p10": float(np.percentile(e, 10)), "median": float(np.median(e)), "mean": float(e.mean()), "max": int(e.max())}


def quench_report(mcq_amd, torch, N, states, sweep_energy, reps):
    """states: uint8 tensor [n][N*N] on the device; sweep_energy: what the sweep reported for them (NumPy)."""
    import numpy as np

    st = torch.cuda.current_stream()
    quench = mcq_amd.quench
    quench.quench_device(N, states, stream=st)  # warm-up
    st.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms, res = [], None
    for _ in range(reps):
        e0.record(st)
        res = quench.quench_device(N, states, stream=st)
        e1.record(st)
        st.synchronize()
        ms.append(e0.elapsed_time(e1))
    e0.record(st)
    quench.quench_device(N, states, conflicts=False, stream=st)
    e1.record(st)
    st.synchronize()
    got = quench.to_numpy(res)
    moves, passes = got["n_moves"], got["n_passes"]
    return {"recount_equals_sweep": bool(np.array_equal(got["energy_in"], sweep_energy)), "before": quantiles(got["energy_in"]), "after": quantiles(got["energy_out"]),
            "already_local_minima": float((moves == 0).mean()), "lowered": float((got["energy_out"] < got["energy_in"]).mean()),
            "moves_per_chain": {"mean": float(moves.mean()), "max": int(moves.max())}, "passes_per_chain": {"mean": float(passes.mean()), "max": int(passes.max())},
            "mean_drop": float((got["energy_in"] - got["energy_out"]).mean()), "max_drop": int((got["energy_in"] - got["energy_out"]).max()),
            "conflict_map_sums_to_2E": bool((got["conflicts"].astype(np.int64).sum(axis=1) == 2 * got["energy_out"]).all()),
            "quench_kernel_ms": min(ms), "quench_kernel_ms_all": ms, "quench_kernel_ms_without_conflict_map": e0.elapsed_time(e1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=65536)
    ap.add_argument("--n-steps", type=int, default=100000)
    ap.add_argument("--resample-every", type=int, default=1000)
    ap.add_argument("--Ns", type=int, nargs="+", default=[12, 15])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    import mcq_amd

    abi, pop = mcq_amd.abi, mcq_amd.population
    if mcq_amd._lib.device_count() < 1:
        raise RuntimeError("quench_study needs a GPU")
    sp = {"type": "linear_annealing", "beta_start": 1.0, "beta_end": 3.0}
    st = torch.cuda.current_stream()
    dev = torch.device("cuda", torch.cuda.current_device())
    n, T, S = args.chains, args.n_steps, args.resample_every
    seeds = abi.seeds_for(42, n)
    report = {"chains": n, "n_steps": T, "resample_every": S, "device": torch.cuda.get_device_name(dev), "cases": []}
    for N in args.Ns:
        case = {"N": N}
        run = mcq_amd._lib.DeviceRun(abi.make_params(N, T, "random", sp, n, mcmc_type="board", trace=False), seeds, trace=False)
        run.launch(st)
        st.synchronize()
        init_ms, sweep_ms = run.launch_timed(st)
        plain = run.results()
        case["plain"] = {"init_kernel_ms": init_ms, "sweep_kernel_ms": sweep_ms}
        for which in ("best", "final"):
            r = quench_report(mcq_amd, torch, N, run.t[which + "_state"], plain[which + "_energy"], args.reps)
            r["share_of_sweep"] = r["quench_kernel_ms"] / sweep_ms
            case["plain"][which + "_state"] = r
        del run
        tm = {}
        pop.anneal_population(N, T, "random", sp, seeds, S, mcmc_type="board", trace=False, timings=tm)  # warm-up
        res, _ = pop.anneal_population(N, T, "random", sp, seeds, S, mcmc_type="board", trace=False, timings=tm)
        case["population"] = {"wall_ms": tm["run_seconds"] * 1e3}
        tq = {}
        resq, _ = pop.anneal_population(N, T, "random", sp, seeds, S, mcmc_type="board", trace=False, timings=tq, quench=True)
        case["population"]["wall_ms_with_quench_hook"] = tq["run_seconds"] * 1e3
        for which in ("best", "final"):
            r = quench_report(mcq_amd, torch, N, torch.from_numpy(res[which + "_state"]).to(dev), res[which + "_energy"], args.reps)
            r["share_of_run"] = r["quench_kernel_ms"] / case["population"]["wall_ms"]
            case["population"][which + "_state"] = r
        case["population"]["hook_equals_standalone"] = bool((resq["quenched_energy"] == mcq_amd.quench.quench_states(N, res["best_state"])["energy_out"]).all())
        report["cases"].append(case)
        print(json.dumps(case), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
