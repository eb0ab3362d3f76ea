#!/usr/bin/env python3
"""What path relinking finds between the minima annealing hands back, how high the barrier between two of them is, and what a call
costs, on one MI355X (profiles/relink.md).

    python tools/relink_study.py [--chains 65536] [--Ns 12 15] [--rounds 10 100] [--out FILE.json] [--profile profiles/relink.md]

The setup of tools/hop_study.py and tools/tabu_study.py: board, random init, linear 1 -> 3, seeds 42 + r, no trace.  Per N the best_state
placements of
  - the heat-bath run resampled as population annealing does (700 sweeps every 7 at N = 12, 445 every 4 at N = 15), and
  - the population annealing run of --n-steps Metropolis steps resampled every --resample-every
are each relinked with a partner from the same pool: the slot before (torch.roll by 1; behind a resampled run that is often a copy of
the same ancestor, a few moves away) and the slot half the pool away.  Recorded per case and partner:
  - d0 (distance_in) to the neighbour as it is, and to its nearest image (quench.nearest_image);
  - one relink_device call on the aligned guides (min_dist = N^2 / 8, pair-move search): the barrier path_max_energy - energy_in, the
    share of pairs whose energy_out lies below both endpoints, min / p10 / median of energy_out, and the milliseconds of the call by
    HIP events (--inner calls back to back in a window, the best and the worst of --reps windows after a warm-up);
  - next to that time the expectation it is held against, in two readings: a tabu_device call of round(mean d0) iterations plus one
    quench_pairs_device call on the same placements (whole calls), and d0 times the time per tabu iteration (a call of --time-iters
    iterations less a call of 0) plus the quench_pairs_device call (net of tabu's launch and table build), timed the same way in the
    same process;
  - relink_pool of each of --rounds rounds: min / p10 / median of the pool's energies and the replacements per round, and hop_device
    (kick 2, pair-move search) and tabu_device (tenure 10 + (0 .. 10)) on the same placements with as many hops and iterations as
    take the pool's measured launch time, from their own time per hop and per iteration in the same session.
It also records the compiler's resource table of every instantiation of the kernel (VGPRs, LDS, scratch) from a compile of
csrc/mcq_relink.hip with -Rpass-analysis=kernel-resource-usage; that part needs no GPU (--resources-only).
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


def resources(mcq_amd):
    """{"NP, pairs": {vgprs, sgprs, lds, scratch, occupancy}} from the compiler's remarks."""
    b = mcq_amd.build
    cmd = [b.hipcc()] + [f for f in b.FLAGS if f != "-shared"] + ["-c", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-o", os.devnull, b.RELINK_SOURCES[0]]
    err = subprocess.run(cmd, capture_output=True, text=True).stderr
    out, cur = {}, None
    for line in err.splitlines():
        m = re.search(r"Function Name: \S*mcq_relink_kernelILi(\d+)ELb(\d)E", line)
        if m:
            cur = out.setdefault(f"{int(m.group(1)):02d} {'pairs' if m.group(2) == '1' else 'single'}", {})
        for key, pat in (("vgprs", r" VGPRs: (\d+)"), ("sgprs", r"TotalSGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)")):
            m = re.search(pat, line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    return out


def quantiles(e):
    import numpy as np

    e = np.asarray(e)
    return {"min": int(e.min()), "p10": float(np.percentile(e, 10)), "median": float(np.median(e)), "mean": float(e.mean()), "max": int(e.max())}


def spread(torch, st, reps, call, inner=1):
    """(best, worst) milliseconds per call over `reps` windows of `inner` calls back to back, after a warm-up."""
    call()  # warm-up
    st.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(reps):
        e0.record(st)
        for _ in range(inner):
            call()
        e1.record(st)
        st.synchronize()
        ms.append(e0.elapsed_time(e1) / inner)
    return min(ms), max(ms)


def timed(torch, st, reps, call, inner=1):
    return spread(torch, st, reps, call, inner)[0]


def pairing(mcq_amd, torch, N, states, seeds, args, shift, tabu_iter_ms):
    """One relink call of every placement with the one `shift` slots before it, and the calls its time is held against."""
    import numpy as np

    quench = mcq_amd.quench
    st = torch.cuda.current_stream()
    md = max(1, N * N // 8)
    raw = torch.roll(states, shift, 0).contiguous()
    guides, image, dist = quench.nearest_image(N, states, raw)
    plain = quench.relink_device(N, states, raw, seeds, min_dist=md, max_steps=1)
    res = quench.relink_device(N, states, guides, seeds, min_dist=md, hist=False)
    on_out = quench.quench_pairs_device(N, res["state"], conflicts=False)
    on_best = quench.quench_device(N, res["path_best_state"], conflicts=False)
    st.synchronize()
    got, on_out, on_best = quench.to_numpy(res), quench.to_numpy(on_out), quench.to_numpy(on_best)
    d_plain = plain["distance_in"].cpu().numpy()
    e_guide = np.roll(got["energy_in"], shift)
    checks = {"aligned_distance_is_the_images": bool(np.array_equal(got["distance_in"], dist.cpu().numpy())),
              "state_is_a_fixed_point": bool(not on_out["n_moves"].any() and not on_out["n_pair_moves"].any() and np.array_equal(on_out["energy_in"], got["energy_out"])),
              "path_best_recounts": bool(np.array_equal(on_best["energy_in"], got["path_best_energy"])),
              "search_does_not_rise": bool((got["energy_out"] <= got["path_best_energy"]).all())}
    k = args.inner
    call_ms, call_worst = spread(torch, st, args.reps, lambda: quench.relink_device(N, states, guides, seeds, min_dist=md, stream=st), k)
    single_ms = timed(torch, st, args.reps, lambda: quench.relink_device(N, states, guides, seeds, min_dist=md, local_search="single", stream=st), k)
    walk_iters = max(1, int(round(float(got["distance_in"].mean()))))
    tabu_ms, tabu_worst = spread(torch, st, args.reps, lambda: quench.tabu_device(N, states, seeds, walk_iters, tenure=10, tenure_rand=10, stream=st), k)
    tabu0_ms = timed(torch, st, args.reps, lambda: quench.tabu_device(N, states, seeds, 0, stream=st), k)
    pairs_ms, pairs_worst = spread(torch, st, args.reps, lambda: quench.quench_pairs_device(N, states, conflicts=False, stream=st), k)
    pairs_best_ms = timed(torch, st, args.reps, lambda: quench.quench_pairs_device(N, res["path_best_state"], conflicts=False, stream=st), k)
    return {"shift": shift, "d0_plain": quantiles(d_plain), "d0_aligned": quantiles(got["distance_in"]), "images_used": int(len(np.unique(image.cpu().numpy()))),
           "barrier": quantiles(got["path_max_energy"] - got["energy_in"]), "energy_in": quantiles(got["energy_in"]), "path_best_energy": quantiles(got["path_best_energy"]),
           "energy_out": quantiles(got["energy_out"]), "below_both_share": float(((got["energy_out"] < got["energy_in"]) & (got["energy_out"] < e_guide)).mean()),
           "below_start_share": float((got["energy_out"] < got["energy_in"]).mean()), "search_moves": float((got["n_moves"] + got["n_pair_moves"]).mean()),
           "checks": checks, "call_ms": call_ms, "call_single_ms": single_ms, "walk_iters": walk_iters, "tabu_walk_ms": tabu_ms, "tabu_no_iters_ms": tabu0_ms,
           "quench_pairs_ms": pairs_ms, "quench_pairs_on_path_best_ms": pairs_best_ms, "expected_ms": tabu_ms + pairs_ms, "call_worst_ms": call_worst,
            "expected_worst_ms": tabu_worst + pairs_worst, "tabu_ms_per_iter": tabu_iter_ms, "net_expected_ms": walk_iters * tabu_iter_ms + pairs_ms}


def report(mcq_amd, torch, N, states, seeds, args):
    quench = mcq_amd.quench
    st = torch.cuda.current_stream()
    tabu0_ms = timed(torch, st, args.reps, lambda: quench.tabu_device(N, states, seeds, 0, stream=st))
    tabu_iter_ms = (timed(torch, st, args.reps, lambda: quench.tabu_device(N, states, seeds, args.time_iters, tenure=10, tenure_rand=10, stream=st)) - tabu0_ms) / args.time_iters
    out = {"pairings": [pairing(mcq_amd, torch, N, states, seeds, args, shift, tabu_iter_ms) for shift in (1, states.shape[0] // 2)], "pools": []}
    hop0_ms = timed(torch, st, args.reps, lambda: quench.hop_device(N, states, seeds, 0, stream=st))
    hop_ms = (timed(torch, st, args.reps, lambda: quench.hop_device(N, states, seeds, args.time_hops, kick=2, stream=st)) - hop0_ms) / args.time_hops
    out.update(hop_ms_per_hop=hop_ms, tabu_ms_per_iter=tabu_iter_ms)
    quench.relink_pool(N, states, seeds, 1, stream=st)  # warm-up: torch's allocations of the images
    for rounds in args.rounds:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        pool = quench.relink_pool(N, states, seeds, rounds, stream=st)
        e1.record(st)
        st.synchronize()
        ms = e0.elapsed_time(e1)
        hops = max(1, int(round(ms / max(hop_ms, 1e-6))))
        iters = max(1, int(round(ms / max(tabu_iter_ms, 1e-6))))
        h = quench.hop_device(N, states, seeds, hops, kick=2)
        t = quench.tabu_device(N, states, seeds, iters, tenure=10, tenure_rand=10)
        st.synchronize()
        out["pools"].append({"rounds": rounds, "ms": ms, "energy": quantiles(pool["energy"].cpu().numpy()), "n_replaced": [int(x) for x in pool["n_replaced"]],
                             "best_energy": [int(x) for x in pool["best_energy"]], "hops": hops, "hop_best_energy": quantiles(h["best_energy"].cpu().numpy()),
                             "tabu_iters": iters, "tabu_best_energy": quantiles(t["best_energy"].cpu().numpy())})
    return out


def markdown(rep):
    q = lambda d: f"{d['min']} / {d['p10']:g} / {d['median']:g}"  # noqa: E731
    lines = ["Compiler's resource table of `csrc/mcq_relink.hip` (`-Rpass-analysis=kernel-resource-usage`, gfx950):", "",
             "| instantiation NP, local search | VGPRs | SGPRs | LDS bytes per chain | scratch bytes per lane | waves per SIMD |", "|---|---|---|---|---|---|"]
    for NP, r in sorted(rep["resources"].items()):
        lines.append(f"| {NP.lstrip('0')} | {r.get('vgprs')} | {r.get('sgprs')} | {r.get('lds')} | {r.get('scratch')} | {r.get('occupancy')} |")
    lines += ["", "No instantiation uses scratch." if not any(r.get("scratch") for r in rep["resources"].values()) else "Some instantiations use scratch: see the table."]
    if not rep.get("cases"):
        return "\n".join(lines + ["", "Not measured: no GPU session was had for the figures below the resource table."])
    lines += ["", f"Measured by `tools/relink_study.py` in one session on one {rep['device']}: {rep['chains']} board chains, linear 1 → 3, seeds 42 + r; `best_state` of each "
              "run, each placement relinked with a partner from the same pool, `min_dist` = N²/8, pair-move search. Times per call are HIP events around "
              f"{rep['inner']} calls back to back, the best of {rep['reps']} such windows after a warm-up, with the worst window in brackets where given. The partner is the slot before (`torch.roll` by 1: behind a resampled run often a copy of the same ancestor) and the slot half the "
              "pool away.", "",
              "### Distances, barriers and what the walk finds", "",
              "| N | placements from | partner | d0 as it is, min / p10 / median | d0 to the nearest image | images used | barrier `path_max_energy` − `energy_in`, min / p10 / median (max) | "
              "`energy_in` | `path_best_energy` | `energy_out` | share below both endpoints | share below their start | moves of the local search per chain |",
              "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    cost = ["", "### Milliseconds per call, against the expectation", "",
            "The expectation: a call costs no more than d0 tabu iterations plus one `quench_pairs_device` call on the same placements. Two readings are shown. WHOLE CALLS: a "
            "`tabu_device` call of round(mean d0) iterations plus a `quench_pairs_device` call, which pay two launches and two table builds against relink's one. NET: d0 times "
            f"the time per tabu iteration (from a call of {rep['time_iters']} iterations less a call of 0, same session) plus the one `quench_pairs_device` call, which leaves "
            "tabu's launch and table build out.", "",
            "| N | placements from | partner | `relink_device` ms (pairs) | (single) | round(mean d0) | `tabu_device` of that many iterations, ms | of 0 iterations, ms | "
            "`quench_pairs_device` ms | WHOLE CALLS: the sum | ms per tabu iteration | NET: d0 iterations + `quench_pairs_device` | `quench_pairs_device` on `path_best_state`, ms |",
            "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    pools = ["", "### The pool, next to the hops and tabu search in equal measured launch time", "",
             "| N | placements from | rounds | ms | pool `energy` min / p10 / median | replacements in the first / last round | fewest – most in a round of the first ten | in all | hops | hops `best_energy` | tabu iterations | "
             "tabu `best_energy` |", "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    ok = True
    for case in rep["cases"]:
        for name in ("heatbath", "population"):
            what = case[name]["what"]
            for c in case[name]["pairings"]:
                ok = ok and all(c["checks"].values())
                lines.append(f"| {case['N']} | {what} | {c['shift']} slot{'s' if c['shift'] != 1 else ''} before | {q(c['d0_plain'])} | {q(c['d0_aligned'])} | {c['images_used']} | {q(c['barrier'])} ({c['barrier']['max']}) | {q(c['energy_in'])} | "
                             f"{q(c['path_best_energy'])} | {q(c['energy_out'])} | {c['below_both_share']:.4f} | {c['below_start_share']:.4f} | {c['search_moves']:.2f} |")
                cost.append(f"| {case['N']} | {what} | {c['shift']} slot{'s' if c['shift'] != 1 else ''} before | {c['call_ms']:.2f} ({c['call_worst_ms']:.2f}) | {c['call_single_ms']:.2f} | "
                            f"{c['walk_iters']} | {c['tabu_walk_ms']:.2f} | {c['tabu_no_iters_ms']:.2f} | {c['quench_pairs_ms']:.2f} | {c['expected_ms']:.2f} ({c['expected_worst_ms']:.2f}) | "
                            f"{c['tabu_ms_per_iter']:.4f} | {c['net_expected_ms']:.2f} | {c['quench_pairs_on_path_best_ms']:.2f} |")
            for p in case[name]["pools"]:
                pools.append(f"| {case['N']} | {what} | {p['rounds']} | {p['ms']:.0f} | {q(p['energy'])} | {p['n_replaced'][0]} / {p['n_replaced'][-1]} | {min(p['n_replaced'][:10])} – {max(p['n_replaced'][:10])} | {sum(p['n_replaced'])} | {p['hops']} | "
                             f"{q(p['hop_best_energy'])} | {p['tabu_iters']} | {q(p['tabu_best_energy'])} |")
    lines += cost + pools
    lines += ["", "In every case the distance of the aligned call is the one `nearest_image` reports, `quench_pairs_device` moves nothing on `state` and recounts `energy_out`, "
              "`quench_device` recounts `path_best_energy` on `path_best_state`, and `energy_out` ≤ `path_best_energy`." if ok else "NOT every case passed the invariants: see the JSON."]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=65536)
    ap.add_argument("--Ns", type=int, nargs="+", default=[12, 15])
    ap.add_argument("--n-steps", type=int, default=100000)
    ap.add_argument("--resample-every", type=int, default=1000)
    ap.add_argument("--rounds", type=int, nargs="+", default=[10, 100])
    ap.add_argument("--time-hops", type=int, default=20)
    ap.add_argument("--time-iters", type=int, default=1000)
    ap.add_argument("--inner", type=int, default=20, help="calls back to back in one timed window of the per-call figures")
    ap.add_argument("--reps", type=int, default=5)
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
            raise RuntimeError("relink_study needs a GPU (or --resources-only)")
        sp = {"type": "linear_annealing", "beta_start": 1.0, "beta_end": 3.0}
        dev = torch.device("cuda", torch.cuda.current_device())
        n = args.chains
        seeds = abi.seeds_for(42, n)
        dseeds = torch.from_numpy(np.ascontiguousarray(seeds, dtype=np.uint32).view(np.int32)).to(dev)
        rep.update(chains=n, n_steps=args.n_steps, resample_every=args.resample_every, reps=args.reps, inner=args.inner, time_iters=args.time_iters, device=torch.cuda.get_device_name(dev))
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
