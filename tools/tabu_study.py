#!/usr/bin/env python3
"""What tabu search finds below the minima annealing hands back, and what an iteration costs, on one MI355X (profiles/tabu.md).

    python tools/tabu_study.py [--chains 65536] [--Ns 12 15] [--iters 1000 10000] [--out FILE.json] [--profile profiles/tabu.md]

The setup of tools/hop_study.py: board, random init, linear 1 -> 3, seeds 42 + r, no trace.  Per N the best_state placements of
  - the heat-bath run resampled as population annealing does (700 sweeps every 7 at N = 12, 445 every 4 at N = 15), and
  - the population annealing run of --n-steps Metropolis steps resampled every --resample-every
go through tabu_device for each of --iters iterations and each tenure of TENURES.  Recorded per case:
  - min / median of energy_in and of best_energy and the share of chains whose best_energy lies below energy_in; moves, uphill moves,
    aspired moves and stalls per iteration;
  - milliseconds of the call by HIP events (best of --reps after a warm-up), less a call of 0 iterations, per iteration;
  - next to it hop_states (kick 2, pair-move search, slack 0) on the same placements with as many hops as take the same launch time,
    from its own time per hop measured in the same session.
It also records the compiler's resource table of every instantiation of the kernel (VGPRs, LDS, scratch) from a compile of
csrc/mcq_tabu.hip with -Rpass-analysis=kernel-resource-usage; that part needs no GPU (--resources-only).
With --profile the section between the two `study` markers of that file is replaced by the tables."""
import argparse
import json
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BEGIN, END = "<!-- study:begin -->", "<!-- study:end -->"
SWEEPS = {12: (700, 7), 15: (445, 4)}
TENURES = ((2, 0, 0), (5, 5, 0), (10, 10, 0), (0, 9, 10), (40, 20, 0))  # (tenure, tenure_rand, tenure_conf); the fourth is TabuCol's rand(0 .. 9) + 0.6 F


def resources(mcq_amd):
    """{NP: {vgprs, sgprs, lds, scratch, occupancy}} from the compiler's remarks."""
    b = mcq_amd.build
    cmd = [b.hipcc()] + [f for f in b.FLAGS if f != "-shared"] + ["-c", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-o", os.devnull, b.TABU_SOURCES[0]]
    err = subprocess.run(cmd, capture_output=True, text=True).stderr
    out, cur = {}, None
    for line in err.splitlines():
        m = re.search(r"Function Name: \S*mcq_tabu_kernelILi(\d+)E", line)
        if m:
            cur = out.setdefault(int(m.group(1)), {})
        for key, pat in (("vgprs", r" VGPRs: (\d+)"), ("sgprs", r"TotalSGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)")):
            m = re.search(pat, line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    return out


def quantiles(e):
    import numpy as np

    return {"min": int(e.min()), "median": float(np.median(e)), "mean": float(e.mean())}


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
    return min(ms)


def report(mcq_amd, torch, N, states, seeds, args):
    import numpy as np

    quench = mcq_amd.quench
    st = torch.cuda.current_stream()
    zero_ms = timed(torch, st, args.reps, lambda: quench.tabu_device(N, states, seeds, 0, stream=st))
    hop0_ms = timed(torch, st, args.reps, lambda: quench.hop_device(N, states, seeds, 0, stream=st))
    hop_ms = (timed(torch, st, args.reps, lambda: quench.hop_device(N, states, seeds, args.time_hops, kick=2, stream=st)) - hop0_ms) / args.time_hops
    rows = []
    for iters in args.iters:
        for tenure, rand, conf in TENURES:
            kw = dict(tenure=tenure, tenure_rand=rand, tenure_conf=conf)
            ms = timed(torch, st, args.reps, lambda: quench.tabu_device(N, states, seeds, iters, stream=st, **kw))
            res = quench.tabu_device(N, states, seeds, iters, hist=iters <= 1000, **kw)
            on_best = quench.quench_device(N, res["best_state"], conflicts=False)
            st.synchronize()
            got, on_best = quench.tabu_to_numpy(res), quench.to_numpy(on_best)
            applies = got["best_iter"] < iters
            checks = {"best_state_recounts": bool(np.array_equal(on_best["energy_in"], got["best_energy"])),
                      "best_state_is_minimum": bool(not on_best["n_moves"][applies].any()),
                      "moves_and_stalls_add_up": bool((got["n_moves"] + got["n_stalled"] == iters).all())}
            if "energy_hist" in got:
                checks["best_is_min_of_hist"] = bool(np.array_equal(got["best_energy"], got["energy_hist"].min(axis=1)))
            per = float(iters * len(got["n_moves"]))
            rows.append({"iters": iters, "tenure": tenure, "tenure_rand": rand, "tenure_conf": conf, "ms": ms, "ms_per_iter": (ms - zero_ms) / iters,
                         "energy_in": quantiles(got["energy_in"]), "best_energy": quantiles(got["best_energy"]), "energy_out": quantiles(got["energy_out"]),
                         "below_start_share": float((got["best_energy"] < got["energy_in"]).mean()), "moves": got["n_moves"].sum() / per,
                         "uphill": got["n_uphill"].sum() / per, "aspired": got["n_aspired"].sum() / per, "stalled": got["n_stalled"].sum() / per, "checks": checks})
        hops = max(1, int(round(min(r["ms"] for r in rows if r["iters"] == iters) / max(hop_ms, 1e-6))))
        h = quench.hop_device(N, states, seeds, hops, kick=2)
        st.synchronize()
        h = quench.to_numpy(h)
        rows.append({"iters": iters, "hops": hops, "hop_energy_start": quantiles(h["energy_start"]), "hop_best_energy": quantiles(h["best_energy"]),
                     "hop_below_start_share": float((h["best_energy"] < h["energy_in"]).mean())})
    return {"rows": rows, "tabu_no_iters_ms": zero_ms, "hop_ms_per_hop": hop_ms, "hop_no_hops_ms": hop0_ms}


def markdown(rep):
    q = lambda d: f"{d['min']} / {d['median']:g}"  # noqa: E731
    lines = ["Compiler's resource table of `csrc/mcq_tabu.hip` (`-Rpass-analysis=kernel-resource-usage`, gfx950):", "",
             "| instantiation NP | VGPRs | SGPRs | LDS bytes per chain | scratch bytes per lane | waves per SIMD |", "|---|---|---|---|---|---|"]
    for NP, r in sorted(rep["resources"].items(), key=lambda kv: int(kv[0])):
        lines.append(f"| {NP} | {r.get('vgprs')} | {r.get('sgprs')} | {r.get('lds')} | {r.get('scratch')} | {r.get('occupancy')} |")
    if not rep.get("cases"):
        return "\n".join(lines)
    lines += ["", f"Measured by `tools/tabu_study.py` in one session on one {rep['device']}: {rep['chains']} board chains, linear 1 → 3, seeds 42 + r; `best_state` of each run "
              "through `tabu_device`. Times are HIP events around one call, best of " f"{rep['reps']} after a warm-up, less a call of 0 iterations.", "",
              "| N | placements from | iterations | tenure + rand + conf/16·F | ms | ms per iteration | `energy_in` min / median | `best_energy` min / median | share of chains below "
              "their start | moves / uphill / aspired / stalled per iteration |", "|---|---|---|---|---|---|---|---|---|---|"]
    hop_lines = ["", "`hop_device` (kick 2, pair-move search, slack 0) on the same placements, with as many hops as fit the fastest tabu launch of that many iterations, from its own "
                 "time per hop in the same session:", "",
                 "| N | placements from | ms per hop | launch time of … tabu iterations | hops | `energy_start` min / median | `best_energy` min / median | share of chains below their input |",
                 "|---|---|---|---|---|---|---|---|"]
    ok = True
    for case in rep["cases"]:
        for name in ("heatbath", "population"):
            c = case[name]
            for r in c["rows"]:
                if "hops" in r:
                    hop_lines.append(f"| {case['N']} | {c['what']} | {c['hop_ms_per_hop']:.3f} | {r['iters']} | {r['hops']} | {q(r['hop_energy_start'])} | {q(r['hop_best_energy'])} | "
                                     f"{r['hop_below_start_share']:.4f} |")
                    continue
                ok = ok and all(r["checks"].values())
                lines.append(f"| {case['N']} | {c['what']} | {r['iters']} | {r['tenure']} + (0 … {r['tenure_rand']}) + {r['tenure_conf']}/16·F | {r['ms']:.1f} | {r['ms_per_iter']:.4f} | "
                             f"{q(r['energy_in'])} | {q(r['best_energy'])} | {r['below_start_share']:.4f} | {r['moves']:.3f} / {r['uphill']:.3f} / {r['aspired']:.4f} / {r['stalled']:.3f} |")
    lines += hop_lines
    lines += ["", "In every case `quench_device` recounts `best_energy` on `best_state`, moves nothing on a `best_state` behind which an iteration ran, moves and stalls add up to the "
              "iterations and, where the history was kept, `best_energy` is its minimum." if ok else "NOT every case passed the invariants: see the JSON."]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=65536)
    ap.add_argument("--Ns", type=int, nargs="+", default=[12, 15])
    ap.add_argument("--n-steps", type=int, default=100000)
    ap.add_argument("--resample-every", type=int, default=1000)
    ap.add_argument("--iters", type=int, nargs="+", default=[1000, 10000])
    ap.add_argument("--time-hops", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--resources-only", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile", default=None)
    args = ap.parse_args()

    import mcq_amd

    rep = {"resources": resources(mcq_amd), "cases": []}
    if not args.resources_only:
        import numpy as np
        import torch

        abi = mcq_amd.abi
        if mcq_amd._lib.device_count() < 1:
            raise RuntimeError("tabu_study needs a GPU (or --resources-only)")
        sp = {"type": "linear_annealing", "beta_start": 1.0, "beta_end": 3.0}
        dev = torch.device("cuda", torch.cuda.current_device())
        n = args.chains
        seeds = abi.seeds_for(42, n)
        dseeds = torch.from_numpy(np.ascontiguousarray(seeds, dtype=np.uint32).view(np.int32)).to(dev)
        rep.update(chains=n, n_steps=args.n_steps, resample_every=args.resample_every, reps=args.reps, device=torch.cuda.get_device_name(dev))
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
    else:
        print(markdown(rep))


if __name__ == "__main__":
    main()
