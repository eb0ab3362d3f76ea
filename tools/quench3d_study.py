#!/usr/bin/env python3
"""What the quench of full_3d placements finds below the placements annealing hands back, and what it costs, on one MI355X
(profiles/quench3d.md).

    python tools/quench3d_study.py [--shapes 12:65536:100000 16:1024:100000 24:1024:20000] [--reps 3] [--out FILE.json]

full_3d, random init, exponential 1 -> 3, seeds 42 + r (the schedule of bench.py --config c3), no trace.  Per shape N:chains:steps, for
best_state and final_state of one launch of the sweep:
  - whether energy_in (the device recount) equals the sweep's own best_energy / final_energy for every chain;
  - the share of placements that were local minima already (n_moves == 0), moves and passes per chain;
  - min / p10 / median energy before and after the quench;
  - the time of one quench call by HIP events (best of --reps, after a warm-up call), with and without the conflict map, next to the
    sweep kernel's time from the same process."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def quantiles(e):
    import numpy as np

    return {"min": int(e.min()), "p10": float(np.percentile(e, 10)), "median": float(np.median(e)), "mean": float(e.mean()), "max": int(e.max())}


def quench_report(mcq_amd, torch, N, states, sweep_energy, reps):
    """states: uint8 tensor [n][3 Q] on the device; sweep_energy: what the sweep reported for them (NumPy)."""
    import numpy as np

    st = torch.cuda.current_stream()
    quench = mcq_amd.quench
    quench.quench_queens_device(N, states, stream=st)  # warm-up
    st.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms, res = [], None
    for _ in range(reps):
        e0.record(st)
        res = quench.quench_queens_device(N, states, stream=st)
        e1.record(st)
        st.synchronize()
        ms.append(e0.elapsed_time(e1))
    e0.record(st)
    quench.quench_queens_device(N, states, conflicts=False, stream=st)
    e1.record(st)
    st.synchronize()
    no_map_ms = e0.elapsed_time(e1)
    e0.record(st)
    quench.quench_queens_device(N, res["state"], stream=st)  # local minima in: the recount and one moveless pass
    e1.record(st)
    st.synchronize()
    got = quench.to_numpy(res)
    moves, passes = got["n_moves"], got["n_passes"]
    return {"recount_equals_sweep": bool(np.array_equal(got["energy_in"], sweep_energy)), "flagged": int((got["flags"] != 0).sum()),
            "before": quantiles(got["energy_in"]), "after": quantiles(got["energy_out"]),
            "already_local_minima": float((moves == 0).mean()), "lowered": float((got["energy_out"] < got["energy_in"]).mean()),
            "moves_per_chain": {"mean": float(moves.mean()), "max": int(moves.max())}, "passes_per_chain": {"mean": float(passes.mean()), "max": int(passes.max())},
            "mean_drop": float((got["energy_in"] - got["energy_out"]).mean()), "max_drop": int((got["energy_in"] - got["energy_out"]).max()),
            "conflict_map_sums_to_2E": bool((got["conflicts"].astype(np.int64).sum(axis=1) == 2 * got["energy_out"]).all()),
            "quench_ms": min(ms), "quench_ms_all": ms, "quench_ms_without_conflict_map": no_map_ms, "quench_ms_of_local_minima": e0.elapsed_time(e1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["12:65536:100000", "16:1024:100000", "24:1024:20000"], help="N:chains:steps")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    import mcq_amd

    abi = mcq_amd.abi
    if mcq_amd._lib.device_count() < 1:
        raise RuntimeError("quench3d_study needs a GPU")
    sp = {"type": "exponential_annealing", "beta_start": 1.0, "beta_end": 3.0}
    st = torch.cuda.current_stream()
    dev = torch.device("cuda", torch.cuda.current_device())
    report = {"device": torch.cuda.get_device_name(dev), "schedule": sp, "cases": []}
    for shape in args.shapes:
        N, n, T = (int(x) for x in shape.split(":"))
        case = {"N": N, "chains": n, "n_steps": T}
        run = mcq_amd._lib.DeviceRun(abi.make_params(N, T, "random", sp, n, mcmc_type="full_3d", trace=False), abi.seeds_for(42, n), trace=False)
        run.launch(st)
        st.synchronize()
        init_ms, sweep_ms = run.launch_timed(st)
        plain = run.results()
        case["init_kernel_ms"], case["sweep_kernel_ms"] = init_ms, sweep_ms
        for which in ("best", "final"):
            r = quench_report(mcq_amd, torch, N, run.t[which + "_state"], plain[which + "_energy"], args.reps)
            r["share_of_sweep"] = r["quench_ms"] / sweep_ms
            case[which + "_state"] = r
        del run
        report["cases"].append(case)
        print(json.dumps(case), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
