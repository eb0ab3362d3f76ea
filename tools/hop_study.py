#!/usr/bin/env python3
"""What basin hopping finds below the minima annealing hands back, and what a hop costs, on one MI355X (profiles/hops.md).

    python tools/hop_study.py [--chains 65536] [--Ns 12 15] [--hops 100] [--time-hops 20] [--out FILE.json] [--profile profiles/hops.md]

Board, random init, linear 1 -> 3, seeds 42 + r, no trace: the shapes of the README.  Per N the best_state placements of
  - the heat-bath run resampled as population annealing does (700 sweeps every 7 at N = 12, 445 every 4 at N = 15), and
  - the population annealing run of --n-steps Metropolis steps resampled every --resample-every
go through hop_device, --hops hops, slack 0, for kick in {1, 2, 4, N} and both local searches.  Recorded per case:
  - min / p10 / median of energy_start (behind the first local search) and of best_energy; n_accepted / n_hops; n_improved; the share of
    chains whose best_energy lies below energy_start;
  - the invariants a batch of this size is checked by: best_energy = the minimum of energy_hist, the history never rises (slack 0),
    state and best_state are fixed points of the local search (the quench kernels move nothing on them) with the energies reported;
  - for kick = 2 and the pair-move search, milliseconds of ONE call of --time-hops hops by HIP events (best of --reps after a warm-up),
    and in the same process on the same placements the only way to do the same work without the kernel: per hop a kick on torch
    tensors (scatter of random heights), quench_pairs_device, and torch.where on the energies.  The composed form draws its kicks
    from torch's generator, so it walks other minima: it is the same work, not the same run.
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

    return {"min": int(e.min()), "p10": float(np.percentile(e, 10)), "median": float(np.median(e)), "mean": float(e.mean())}


def timed(torch, st, reps, call):
    call()  # warm-up
    st.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(reps):
        e0.record(st)
        call()
        e1.record(st)
        st.synchronize()
        ms.append(e0.elapsed_time(e1))
    return min(ms), ms


def composed(mcq_amd, torch, N, states, hops, kick, slack, gen):
    """The same work from the calls the library had before mcq_hop: a launch, a host-side kick and a select per hop."""
    quench = mcq_amd.quench
    n, Q = states.shape
    first = quench.quench_pairs_device(N, states, conflicts=False)
    cur, E = first["state"], first["energy_out"]
    for _ in range(hops):
        idx = torch.randint(0, Q, (n, kick), device=states.device, generator=gen)
        val = torch.randint(0, N, (n, kick), device=states.device, generator=gen).to(torch.uint8)
        r = quench.quench_pairs_device(N, cur.scatter(1, idx, val), conflicts=False)
        keep = r["energy_out"] <= E + slack
        cur, E = torch.where(keep[:, None], r["state"], cur), torch.where(keep, r["energy_out"], E)
    return cur, E


def hop_case(mcq_amd, torch, N, states, seeds, hops, kick, search):
    import numpy as np

    quench = mcq_amd.quench
    st = torch.cuda.current_stream()
    res = quench.hop_device(N, states, seeds, hops, kick=kick, slack=0, local_search=search, hist=True)
    L = (lambda s: quench.quench_pairs_device(N, s, conflicts=False)) if search == "pairs" else (lambda s: quench.quench_device(N, s, conflicts=False))
    on_state, on_best = L(res["state"]), L(res["best_state"])
    st.synchronize()
    got, on_state, on_best = quench.to_numpy(res), quench.to_numpy(on_state), quench.to_numpy(on_best)
    hist = got["energy_hist"].astype(np.int64)
    fixed = lambda q, e: bool(not q["n_moves"].any() and not q.get("n_pair_moves", np.zeros(1)).any() and np.array_equal(q["energy_in"], e))  # noqa: E731
    return {"kick": kick, "local_search": search, "hops": hops,
            "energy_in": quantiles(got["energy_in"]), "energy_start": quantiles(got["energy_start"]), "best_energy": quantiles(got["best_energy"]),
            "energy_out": quantiles(got["energy_out"]),
            "accepted_share": float(got["n_accepted"].sum()) / float(max(hops, 1) * len(hist)), "n_improved": int(got["n_improved"].sum()),
            "chains_improved_share": float((got["best_energy"] < got["energy_start"]).mean()),
            "moves_per_hop": float(got["n_moves"].sum()) / float(max(hops, 1) * len(hist)),
            "pair_moves_per_hop": float(got["n_pair_moves"].sum()) / float(max(hops, 1) * len(hist)),
            "checks": {"best_is_min_of_hist": bool(np.array_equal(got["best_energy"], hist.min(axis=1)) and np.array_equal(got["best_hop"], hist.argmin(axis=1))),
                       "hist_never_rises": bool((np.diff(hist, axis=1) <= 0).all()),
                       "state_is_fixed_point": fixed(on_state, got["energy_out"]), "best_state_is_fixed_point": fixed(on_best, got["best_energy"])}}


def report(mcq_amd, torch, N, states, seeds, args):
    st = torch.cuda.current_stream()
    quench = mcq_amd.quench
    rows = [hop_case(mcq_amd, torch, N, states, seeds, args.hops, kick, search) for search in ("single", "pairs") for kick in (1, 2, 4, N)]
    k = args.time_hops
    gen = torch.Generator(device=states.device)
    gen.manual_seed(1)
    one_ms, one_all = timed(torch, st, args.reps, lambda: quench.hop_device(N, states, seeds, k, kick=2, slack=0, local_search="pairs", stream=st))
    comp_ms, comp_all = timed(torch, st, args.reps, lambda: composed(mcq_amd, torch, N, states, k, 2, 0, gen))
    zero_ms, _ = timed(torch, st, args.reps, lambda: quench.hop_device(N, states, seeds, 0, kick=2, slack=0, local_search="pairs", stream=st))
    return {"rows": rows, "time_hops": k, "hop_device_ms": one_ms, "hop_device_ms_all": one_all, "composed_ms": comp_ms, "composed_ms_all": comp_all,
            "hop_device_no_hops_ms": zero_ms, "hop_device_ms_per_hop": (one_ms - zero_ms) / k, "composed_ms_per_hop": comp_ms / k, "ratio": one_ms / comp_ms}


def markdown(rep):
    q = lambda d: f"{d['min']} / {d['p10']:g} / {d['median']:g}"  # noqa: E731
    lines = [f"Measured by `tools/hop_study.py` in one session on one {rep['device']}: {rep['chains']} board chains, linear 1 → 3, seeds 42 + r; `best_state` of "
             f"each run through `hop_device`, {rep['hops']} hops, slack 0.", "",
             "| N | placements from | local search | kick | `energy_start` min / p10 / median | `best_energy` min / p10 / median | accepted / hops | `n_improved` (all chains) | "
             "share of chains improved | single / pair moves per hop |", "|---|---|---|---|---|---|---|---|---|---|"]
    for case in rep["cases"]:
        for name in ("heatbath", "population"):
            for r in case[name]["rows"]:
                lines.append(f"| {case['N']} | {case[name]['what']} | {r['local_search']} | {r['kick']} | {q(r['energy_start'])} | {q(r['best_energy'])} | "
                             f"{r['accepted_share']:.3f} | {r['n_improved']} | {r['chains_improved_share']:.4f} | {r['moves_per_hop']:.2f} / {r['pair_moves_per_hop']:.3f} |")
    ok = all(all(r["checks"].values()) for case in rep["cases"] for n in ("heatbath", "population") for r in case[n]["rows"])
    lines += ["", "In every case `best_energy` / `best_hop` are the first minimum of `energy_hist`, the history never rises, and the quench kernels move nothing on any `state` or "
              "`best_state` and recount the energies reported." if ok else "NOT every case passed the invariants: see the JSON.", "",
              f"Time of one call of {rep['time_hops']} hops (kick 2, pair-move search), HIP events, best of {rep['reps']} after a warm-up call, against the composed calls (per hop a "
              "kick on torch tensors, `quench_pairs_device`, `torch.where`) in the same process on the same placements. The composed form draws its kicks from torch's "
              "generator: the same work, not the same run.", "",
              "| N | placements from | `hop_device` ms | of which the first local search (a call of 0 hops) | ms per hop | composed ms | composed ms per hop | ratio |",
              "|---|---|---|---|---|---|---|---|"]
    for case in rep["cases"]:
        for name in ("heatbath", "population"):
            r = case[name]
            lines.append(f"| {case['N']} | {r['what']} | {r['hop_device_ms']:.2f} | {r['hop_device_no_hops_ms']:.2f} | {r['hop_device_ms_per_hop']:.3f} | {r['composed_ms']:.2f} | "
                         f"{r['composed_ms_per_hop']:.3f} | {r['ratio']:.2f} |")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=65536)
    ap.add_argument("--Ns", type=int, nargs="+", default=[12, 15])
    ap.add_argument("--n-steps", type=int, default=100000)
    ap.add_argument("--resample-every", type=int, default=1000)
    ap.add_argument("--hops", type=int, default=100)
    ap.add_argument("--time-hops", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    import mcq_amd

    abi = mcq_amd.abi
    if mcq_amd._lib.device_count() < 1:
        raise RuntimeError("hop_study needs a GPU")
    sp = {"type": "linear_annealing", "beta_start": 1.0, "beta_end": 3.0}
    dev = torch.device("cuda", torch.cuda.current_device())
    n = args.chains
    seeds = abi.seeds_for(42, n)
    dseeds = torch.from_numpy(np.ascontiguousarray(seeds, dtype=np.uint32).view(np.int32)).to(dev)
    rep = {"chains": n, "n_steps": args.n_steps, "resample_every": args.resample_every, "hops": args.hops, "time_hops": args.time_hops, "reps": args.reps,
           "device": torch.cuda.get_device_name(dev), "cases": []}
    for N in args.Ns:
        sweeps, every = SWEEPS.get(N, (500, 5))
        case = {"N": N}
        res, _ = mcq_amd.heatbath.anneal_heatbath(N, sweeps, "random", sp, seeds, resample_every=every)
        case["heatbath"] = dict(report(mcq_amd, torch, N, torch.from_numpy(res["best_state"]).to(dev), dseeds, args), what=f"heat bath, {sweeps} sweeps, resampled every {every}")
        print(json.dumps({"N": N, "heatbath": case["heatbath"]}), flush=True)
        res, _ = mcq_amd.population.anneal_population(N, args.n_steps, "random", sp, seeds, args.resample_every, mcmc_type="board", trace=False)
        case["population"] = dict(report(mcq_amd, torch, N, torch.from_numpy(res["best_state"]).to(dev), dseeds, args),
                                  what=f"population annealing, {args.n_steps} steps, resampled every {args.resample_every}")
        print(json.dumps({"N": N, "population": case["population"]}), flush=True)
        rep["cases"].append(case)
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
