#!/usr/bin/env python3
"""What the pair-move quench finds below the single-move minima annealing hands back, and what it costs, on one MI355X
(profiles/quench_pairs.md).

    python tools/quench_pairs_study.py [--chains 65536] [--Ns 12 15] [--out FILE.json] [--profile profiles/quench_pairs.md]

Board, random init, linear 1 -> 3, seeds 42 + r, no trace: the shapes of the README.  Per N the best_state placements of
  - the heat-bath run resampled as population annealing does (700 sweeps every 7 at N = 12, 445 every 4 at N = 15; --sweeps / --every), and
  - the population annealing run of --n-steps Metropolis steps resampled every --resample-every
go through quench_pairs_device and, in the same process on the same placements, through quench_device.  Recorded per case:
  - milliseconds per call by HIP events (best of --reps after a warm-up call, without the conflict map), both kernels and their ratio;
  - rounds and pair moves per chain; min / p10 / median of energy_single and energy_out; the share of chains with energy_out < energy_single;
  - whether energy_single equals quench_device's energy_out and the single-move quench moves nothing on the output, for every chain.
With --profile the section between the two `study` markers of that file is replaced by the tables."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BEGIN, END = "<!-- study:begin -->", "<!-- study:end -->"
SWEEPS = {12: (700, 7), 15: (445, 4)}


def quantiles(e):
    import numpy as np

    return {"min": int(e.min()), "p10": float(np.percentile(e, 10)), "median": float(np.median(e)), "mean": float(e.mean()), "max": int(e.max())}


def timed(torch, st, reps, call):
    call()  # warm-up
    st.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms, res = [], None
    for _ in range(reps):
        e0.record(st)
        res = call()
        e1.record(st)
        st.synchronize()
        ms.append(e0.elapsed_time(e1))
    return min(ms), ms, res


def report(mcq_amd, torch, N, states, reps):
    """states: uint8 tensor [n][N*N] on the device."""
    import numpy as np

    st = torch.cuda.current_stream()
    quench = mcq_amd.quench
    single_ms, single_all, single = timed(torch, st, reps, lambda: quench.quench_device(N, states, conflicts=False, stream=st))
    pairs_ms, pairs_all, pairs = timed(torch, st, reps, lambda: quench.quench_pairs_device(N, states, conflicts=False, stream=st))
    again = quench.quench_device(N, pairs["state"], conflicts=False, stream=st)
    st.synchronize()
    single, got, again = quench.to_numpy(single), quench.to_numpy(pairs), quench.to_numpy(again)
    rounds, pm = got["n_rounds"], got["n_pair_moves"]
    return {"quench_device_ms": single_ms, "quench_device_ms_all": single_all, "quench_pairs_device_ms": pairs_ms, "quench_pairs_device_ms_all": pairs_all,
            "ratio": pairs_ms / single_ms,
            "energy_in": quantiles(got["energy_in"]), "energy_single": quantiles(got["energy_single"]), "energy_out": quantiles(got["energy_out"]),
            "improved_share": float((got["energy_out"] < got["energy_single"]).mean()),
            "single_move_minima_on_entry": float((single["n_moves"] == 0).mean()),
            "rounds_per_chain": {"mean": float(rounds.mean()), "max": int(rounds.max())},
            "pair_moves_per_chain": {"mean": float(pm.mean()), "max": int(pm.max())},
            "mean_drop": float((got["energy_single"] - got["energy_out"]).mean()), "max_drop": int((got["energy_single"] - got["energy_out"]).max()),
            "certified_share": float((got["certified"] == 1).mean()),
            "energy_single_equals_quench_device": bool(np.array_equal(got["energy_single"], single["energy_out"])),
            "output_is_single_move_minimum": bool((again["n_moves"] == 0).all() and np.array_equal(again["energy_in"], got["energy_out"]))}


def markdown(rep):
    q = lambda d: f"{d['min']} / {d['p10']:g} / {d['median']:g}"  # noqa: E731
    lines = [f"Measured by `tools/quench_pairs_study.py` in one session on one {rep['device']}: {rep['chains']} board chains, linear 1 → 3, seeds 42 + r; "
             f"`best_state` of each run; milliseconds by HIP events, best of {rep['reps']} after a warm-up call, both kernels without the conflict map, "
             "in the same process on the same placements.", "",
             "| N | placements from | `quench_device` ms | `quench_pairs_device` ms | ratio | rounds per chain (mean / most) | pair moves per chain (mean / most) | "
             "`energy_single` min / p10 / median | `energy_out` min / p10 / median | share with `energy_out < energy_single` |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for case in rep["cases"]:
        for name in ("heatbath", "population"):
            r = case[name]
            lines.append(f"| {case['N']} | {r['what']} | {r['quench_device_ms']:.2f} | {r['quench_pairs_device_ms']:.2f} | {r['ratio']:.2f} | "
                         f"{r['rounds_per_chain']['mean']:.3f} / {r['rounds_per_chain']['max']} | {r['pair_moves_per_chain']['mean']:.3f} / {r['pair_moves_per_chain']['max']} | "
                         f"{q(r['energy_single'])} | {q(r['energy_out'])} | {r['improved_share']:.4f} |")
    ok = all(case[n]["energy_single_equals_quench_device"] and case[n]["output_is_single_move_minimum"] and case[n]["certified_share"] == 1.0
             for case in rep["cases"] for n in ("heatbath", "population"))
    lines += ["", "In every case `energy_single` equals `quench_device`'s `energy_out` for every chain, the single-move quench moves nothing on any output, and every chain is certified."
              if ok else "NOT every case passed the checks on `energy_single`, the output and `certified`: see the JSON."]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=65536)
    ap.add_argument("--Ns", type=int, nargs="+", default=[12, 15])
    ap.add_argument("--n-steps", type=int, default=100000)
    ap.add_argument("--resample-every", type=int, default=1000)
    ap.add_argument("--sweeps", type=int, default=None, help="heat-bath sweeps (default: 700 at N = 12, 445 at N = 15, 500 elsewhere)")
    ap.add_argument("--every", type=int, default=None, help="heat-bath sweeps between two resamplings (default: 7 / 4 / 5)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile", default=None)
    args = ap.parse_args()

    import torch

    import mcq_amd

    abi = mcq_amd.abi
    if mcq_amd._lib.device_count() < 1:
        raise RuntimeError("quench_pairs_study needs a GPU")
    sp = {"type": "linear_annealing", "beta_start": 1.0, "beta_end": 3.0}
    dev = torch.device("cuda", torch.cuda.current_device())
    n = args.chains
    seeds = abi.seeds_for(42, n)
    rep = {"chains": n, "n_steps": args.n_steps, "resample_every": args.resample_every, "reps": args.reps, "device": torch.cuda.get_device_name(dev), "cases": []}
    for N in args.Ns:
        sweeps, every = SWEEPS.get(N, (500, 5))
        sweeps, every = args.sweeps or sweeps, args.every or every
        case = {"N": N}
        res, _ = mcq_amd.heatbath.anneal_heatbath(N, sweeps, "random", sp, seeds, resample_every=every)
        case["heatbath"] = dict(report(mcq_amd, torch, N, torch.from_numpy(res["best_state"]).to(dev), args.reps),
                                what=f"heat bath, {sweeps} sweeps, resampled every {every}")
        res, _ = mcq_amd.population.anneal_population(N, args.n_steps, "random", sp, seeds, args.resample_every, mcmc_type="board", trace=False)
        case["population"] = dict(report(mcq_amd, torch, N, torch.from_numpy(res["best_state"]).to(dev), args.reps),
                                  what=f"population annealing, {args.n_steps} steps, resampled every {args.resample_every}")
        rep["cases"].append(case)
        print(json.dumps(case), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rep, f, indent=1)
    if args.profile:
        with open(args.profile) as f:
            text = f.read()
        if BEGIN not in text or END not in text:
            raise RuntimeError(f"{args.profile} has no study markers")
        text = text[: text.index(BEGIN) + len(BEGIN)] + "\n" + markdown(rep) + "\n" + text[text.index(END):]
        with open(args.profile, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
