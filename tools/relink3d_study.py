#!/usr/bin/env python3
"""What path relinking finds between full_3d minima, how high the barrier between two of them is, and what a call costs, on one MI355X
(profiles/relink3d.md).

    python tools/relink3d_study.py [--chains 4096] [--Ns 12 15] [--rounds 100] [--out FILE.json] [--profile profiles/relink3d.md]
    python tools/relink3d_study.py --resources-only [--profile profiles/relink3d.md]      (no GPU: the compiler's resource table only)

The setup of tools/tabu3d_study.py: random init, linear 1 -> 3, seeds 42 + r, no trace, Q = N^2.  Per N two pools of placements:
  (a) best_state of tabu_queens (--tabu-iters iterations, tenure 10 + (0 .. 10)) behind the full_3d heat bath (--sweeps queen sweeps);
  (b) the board plateau: best_state of the board heat bath resampled as population annealing does (700 sweeps every 7 at N = 12, 445
      every 4 at N = 15) behind --board-hops board hops with the pair-move search, carried into the cube by queens_of_boards and
      quenched there (quench_queens_device), so that both endpoints of a walk are minima of the cube.
Each placement is relinked with the slot before it (torch.roll by 1) and with the slot half the pool away, with the guide as it is and
with its nearest image (quench.nearest_queens_image), min_dist = Q / 8.  Recorded per case:
  - d0 (distance_in), the barrier path_max_energy - energy_in, energy_in, path_best_energy, energy_out, the share of pairs whose
    energy_out lies below both endpoints and the largest gain among them, the moves of the local search, and the invariants (state is
    a fixed point of quench_queens_device, path_best_state recounts to path_best_energy, energy_out <= path_best_energy);
  - milliseconds of the call by HIP events (--inner calls back to back in a window, the best and the worst of --reps windows after a
    warm-up), alternated window by window with the expectation it is held against, in two readings: WHOLE CALLS, a tabu_queens_device
    call of round(mean d0) iterations plus one quench_queens_device call on the same placements; NET, d0 times the time per tabu
    iteration (a call of --time-iters iterations less a call of 0) plus the quench_queens_device call;
  - relink_queens_pool of --rounds rounds (aligned), and hop_queens_device (kick 2) and tabu_queens_device (tenure 10 + (0 .. 10)) on
    the same placements with as many hops and iterations as take the pool's measured launch time.
It also records the compiler's resource table of the three instantiations from a compile of csrc/mcq_relink3d.hip with
-Rpass-analysis=kernel-resource-usage; that part needs no GPU.  With --profile the section between the two `study` markers of that
file is replaced by the tables."""
import argparse
import json
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BEGIN, END = "<!-- study:begin -->", "<!-- study:end -->"
SWEEPS = {12: (700, 7), 15: (445, 4)}
SHAPE_ENDS = {64: 12, 256: 19, 1024: 32}  # lanes per chain -> the largest N of the instantiation


def resources(mcq_amd):
    """{W: {vgprs, sgprs, sgpr_spill, vgpr_spill, lds, scratch, occupancy}} from the compiler's remarks."""
    b = mcq_amd.build
    cmd = [b.hipcc()] + [f for f in b.FLAGS if f != "-shared"] + ["-c", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-o", os.devnull, b.RELINK3D_SOURCES[0]]
    err = subprocess.run(cmd, capture_output=True, text=True).stderr
    out, cur = {}, None
    for line in err.splitlines():
        m = re.search(r"Function Name: \S*mcq_relink3d_kernelILi(\d+)E", line)
        if m:
            cur = out.setdefault(int(m.group(1)), {})
        for key, pat in (("vgprs", r" VGPRs: (\d+)"), ("sgprs", r"TotalSGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("sgpr_spill", r"SGPRs Spill: (\d+)"), ("vgpr_spill", r"VGPRs Spill: (\d+)"),
                         ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)")):
            m = re.search(pat, line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    return out


def quantiles(e):
    import numpy as np

    e = np.asarray(e)
    return {"min": int(e.min()), "p10": float(np.percentile(e, 10)), "median": float(np.median(e)), "mean": float(e.mean()), "max": int(e.max())}


def alternated(torch, st, reps, inner, calls):
    """{name: (best, worst) milliseconds per call}: `reps` rounds, each one window of `inner` calls back to back per entry of `calls`, the
    entries taking turns within a round, after a warm-up of each."""
    for call in calls.values():
        call()
    st.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = {k: [] for k in calls}
    for _ in range(reps):
        for k, call in calls.items():
            e0.record(st)
            for _ in range(inner):
                call()
            e1.record(st)
            st.synchronize()
            ms[k].append(e0.elapsed_time(e1) / inner)
    return {k: (min(v), max(v)) for k, v in ms.items()}


def pairing(mcq_amd, torch, N, states, seeds, args, shift, align):
    """One relink call of every placement with the one `shift` slots before it, and the calls its time is held against."""
    import numpy as np

    quench = mcq_amd.quench
    st = torch.cuda.current_stream()
    md = max(1, N * N // 8)
    guides = torch.roll(states, shift, 0).contiguous()
    image = None
    if align:
        guides, image, dist = quench.nearest_queens_image(N, states, guides)
    res = quench.relink_queens_device(N, states, guides, seeds, min_dist=md)
    on_out = quench.quench_queens_device(N, res["state"], conflicts=False)
    on_best = quench.quench_queens_device(N, res["path_best_state"], max_passes=1, conflicts=False)
    st.synchronize()
    got, on_out, on_best = quench.to_numpy(res), quench.to_numpy(on_out), quench.to_numpy(on_best)
    e_guide = np.roll(got["energy_in"], shift)
    both = np.minimum(got["energy_in"], e_guide)
    below = got["energy_out"] < both
    checks = {"state_is_a_fixed_point": bool(not on_out["n_moves"].any() and np.array_equal(on_out["energy_in"], got["energy_out"])),
              "path_best_recounts": bool(np.array_equal(on_best["energy_in"], got["path_best_energy"])),
              "search_does_not_rise": bool((got["energy_out"] <= got["path_best_energy"]).all()), "none_flagged": bool(not got["flags"].any())}
    if align:
        checks["aligned_distance_is_the_images"] = bool(np.array_equal(got["distance_in"], dist.cpu().numpy()))
    walk_iters = max(1, int(round(float(got["distance_in"].mean()))))
    t = alternated(torch, st, args.reps, args.inner, {
        "relink": lambda: quench.relink_queens_device(N, states, guides, seeds, min_dist=md, stream=st),
        "tabu_walk": lambda: quench.tabu_queens_device(N, states, seeds, walk_iters, tenure=10, tenure_rand=10, stream=st),
        "tabu_0": lambda: quench.tabu_queens_device(N, states, seeds, 0, stream=st),
        "tabu_long": lambda: quench.tabu_queens_device(N, states, seeds, args.time_iters, tenure=10, tenure_rand=10, stream=st),
        "quench": lambda: quench.quench_queens_device(N, states, conflicts=False, stream=st),
        "quench_on_path_best": lambda: quench.quench_queens_device(N, res["path_best_state"], conflicts=False, stream=st)})
    per_iter = (t["tabu_long"][0] - t["tabu_0"][0]) / args.time_iters
    return {"shift": shift, "aligned": bool(align), "images_used": None if image is None else int(len(np.unique(image.cpu().numpy()))),
            "d0": quantiles(got["distance_in"]), "barrier": quantiles(got["path_max_energy"] - got["energy_in"]), "energy_in": quantiles(got["energy_in"]),
            "path_best_energy": quantiles(got["path_best_energy"]), "energy_out": quantiles(got["energy_out"]), "below_both_share": float(below.mean()),
            "below_both_largest_gain": int((both - got["energy_out"])[below].max()) if below.any() else 0, "below_start_share": float((got["energy_out"] < got["energy_in"]).mean()),
            "search_moves": float(got["n_moves"].mean()), "search_passes": float(got["n_passes"].mean()), "checks": checks, "walk_iters": walk_iters,
            "ms": {k: list(v) for k, v in t.items()}, "tabu_ms_per_iter": per_iter, "expected_ms": t["tabu_walk"][0] + t["quench"][0],
            "net_expected_ms": walk_iters * per_iter + t["quench"][0]}


def report(mcq_amd, torch, N, states, seeds, args):
    quench = mcq_amd.quench
    st = torch.cuda.current_stream()
    out = {"pairings": [pairing(mcq_amd, torch, N, states, seeds, args, shift, align) for shift in (1, states.shape[0] // 2) for align in (False, True)], "pools": []}
    t = alternated(torch, st, args.reps, 1, {"hop_0": lambda: quench.hop_queens_device(N, states, seeds, 0, stream=st),
                                             "hop": lambda: quench.hop_queens_device(N, states, seeds, args.time_hops, kick=2, stream=st),
                                             "tabu_0": lambda: quench.tabu_queens_device(N, states, seeds, 0, stream=st),
                                             "tabu": lambda: quench.tabu_queens_device(N, states, seeds, args.time_iters, tenure=10, tenure_rand=10, stream=st)})
    hop_ms, tabu_ms = (t["hop"][0] - t["hop_0"][0]) / args.time_hops, (t["tabu"][0] - t["tabu_0"][0]) / args.time_iters
    out.update(hop_ms_per_hop=hop_ms, tabu_ms_per_iter=tabu_ms)
    quench.relink_queens_pool(N, states, seeds, 1, stream=st)  # warm-up: torch's allocations of the images
    for rounds in args.rounds:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        pool = quench.relink_queens_pool(N, states, seeds, rounds, stream=st)
        e1.record(st)
        st.synchronize()
        ms = e0.elapsed_time(e1)
        hops, iters = max(1, int(round(ms / max(hop_ms, 1e-6)))), max(1, int(round(ms / max(tabu_ms, 1e-6))))
        h = quench.hop_queens_device(N, states, seeds, hops, kick=2)
        tb = quench.tabu_queens_device(N, states, seeds, iters, tenure=10, tenure_rand=10)
        st.synchronize()
        out["pools"].append({"rounds": rounds, "ms": ms, "energy": quantiles(pool["energy"].cpu().numpy()), "n_replaced": [int(x) for x in pool["n_replaced"]],
                             "best_energy": [int(x) for x in pool["best_energy"]], "hops": hops, "hop_best_energy": quantiles(h["best_energy"].cpu().numpy()),
                             "tabu_iters": iters, "tabu_best_energy": quantiles(tb["best_energy"].cpu().numpy())})
    return out


def markdown(rep):
    q = lambda d: f"{d['min']} / {d['p10']:g} / {d['median']:g}"  # noqa: E731
    lines = ["Compiler's resource table of `csrc/mcq_relink3d.hip` (`-Rpass-analysis=kernel-resource-usage`, gfx950):", "",
             "| lanes per chain (N up to) | VGPRs | SGPRs | VGPRs spilled | SGPRs spilled (to VGPR lanes) | scratch bytes per lane | static LDS bytes | waves per SIMD | dynamic LDS bytes per chain at that N, Q = N² |",
             "|---|---|---|---|---|---|---|---|---|"]
    for W, r in sorted(rep["resources"].items(), key=lambda kv: int(kv[0])):
        N = SHAPE_ENDS[int(W)]
        lines.append(f"| {W} ({N}) | {r.get('vgprs')} | {r.get('sgprs')} | {r.get('vgpr_spill')} | {r.get('sgpr_spill')} | {r.get('scratch')} | {r.get('lds')} | {r.get('occupancy')} | {rep['lds'][str(N)]} |")
    clean = not any(r.get("scratch") or r.get("vgpr_spill") for r in rep["resources"].values())
    lines += ["", "No instantiation uses scratch, and none spills a vector register; the scalar registers the table lists as spilled are kept in lanes of a vector "
              "register, never in memory." if clean else "Some instantiations use scratch or spill vector registers: see the table."]
    if not rep.get("cases"):
        return "\n".join(lines + ["", "Not measured: no GPU session was had for the figures below the resource table."])
    lines += ["", f"Measured by `tools/relink3d_study.py` in one session on one {rep['device']}: {rep['chains']} full_3d chains of N² queens, linear 1 → 3, seeds 42 + r. "
              f"Times per call are HIP events around {rep['inner']} calls back to back, the best of {rep['reps']} such windows after a warm-up with the worst in brackets; the "
              "windows of a call and of what it is held against take turns.", "",
              "### Distances, barriers and what the walk finds", "",
              "| N | placements from | partner | guide | d0 min / p10 / median | images used | barrier min / p10 / median (max) | `energy_in` | `path_best_energy` | `energy_out` | "
              "share below both endpoints | largest gain below both | share below their start | moves (passes) of the local search per chain |",
              "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    cost = ["", "### Milliseconds per call, against the expectation", "",
            "The expectation: a call costs no more than d0 tabu iterations plus one `quench_queens_device` call on the same placements. WHOLE CALLS: a `tabu_queens_device` "
            "call of round(mean d0) iterations plus a `quench_queens_device` call, which pay two launches and two field builds against relink's one. NET: d0 times the time "
            f"per tabu iteration (a call of {rep['time_iters']} iterations less a call of 0) plus the one `quench_queens_device` call.", "",
            "| N | placements from | partner | guide | `relink_queens_device` ms | round(mean d0) | `tabu_queens_device` of that many iterations, ms | of 0 iterations, ms | "
            "`quench_queens_device` ms | WHOLE CALLS: the sum | ms per tabu iteration | NET | `quench_queens_device` on `path_best_state`, ms |",
            "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    pools = ["", "### The pool, next to the hops and tabu search in equal measured launch time", "",
             "| N | placements from | rounds | ms | pool `energy` min / p10 / median | pool's best energy behind the first / last round | replacements in the first / last round | in all | hops | "
             "hops `best_energy` | tabu iterations | tabu `best_energy` |", "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    ok = True
    for case in rep["cases"]:
        for name in ("cube", "plateau"):
            if name not in case:
                continue
            what = case[name]["what"]
            for c in case[name]["pairings"]:
                ok = ok and all(c["checks"].values())
                partner, guide = f"{c['shift']} slot{'s' if c['shift'] != 1 else ''} before", "nearest image" if c["aligned"] else "as it is"
                m = c["ms"]
                lines.append(f"| {case['N']} | {what} | {partner} | {guide} | {q(c['d0'])} | {c['images_used'] if c['aligned'] else '–'} | {q(c['barrier'])} ({c['barrier']['max']}) | "
                             f"{q(c['energy_in'])} | {q(c['path_best_energy'])} | {q(c['energy_out'])} | {c['below_both_share']:.4f} | {c['below_both_largest_gain']} | "
                             f"{c['below_start_share']:.4f} | {c['search_moves']:.2f} ({c['search_passes']:.2f}) |")
                cost.append(f"| {case['N']} | {what} | {partner} | {guide} | {m['relink'][0]:.2f} ({m['relink'][1]:.2f}) | {c['walk_iters']} | {m['tabu_walk'][0]:.2f} ({m['tabu_walk'][1]:.2f}) | "
                            f"{m['tabu_0'][0]:.2f} | {m['quench'][0]:.2f} ({m['quench'][1]:.2f}) | {c['expected_ms']:.2f} | {c['tabu_ms_per_iter']:.4f} | {c['net_expected_ms']:.2f} | "
                            f"{m['quench_on_path_best'][0]:.2f} |")
            for p in case[name]["pools"]:
                pools.append(f"| {case['N']} | {what} | {p['rounds']} | {p['ms']:.0f} | {q(p['energy'])} | {p['best_energy'][0]} / {p['best_energy'][-1]} | {p['n_replaced'][0]} / {p['n_replaced'][-1]} | "
                             f"{sum(p['n_replaced'])} | {p['hops']} | {q(p['hop_best_energy'])} | {p['tabu_iters']} | {q(p['tabu_best_energy'])} |")
    lines += cost + pools
    lines += ["", "In every case `quench_queens_device` moves nothing on `state` and recounts `energy_out`, recounts `path_best_energy` on `path_best_state`, `energy_out` ≤ "
              "`path_best_energy`, no chain is flagged, and the distance of an aligned call is the one `nearest_queens_image` reports." if ok
              else "NOT every case passed the invariants: see the JSON."]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=4096)
    ap.add_argument("--Ns", type=int, nargs="+", default=[12, 15])
    ap.add_argument("--sweeps", type=int, default=200)
    ap.add_argument("--tabu-iters", type=int, default=1000)
    ap.add_argument("--board-hops", type=int, default=1000)
    ap.add_argument("--no-plateau", action="store_true", help="leave the board plateaus out (they take most of the session)")
    ap.add_argument("--rounds", type=int, nargs="+", default=[100])
    ap.add_argument("--time-hops", type=int, default=20)
    ap.add_argument("--time-iters", type=int, default=500)
    ap.add_argument("--inner", type=int, default=3, help="calls back to back in one timed window of the per-call figures")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--resources-only", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile", default=None)
    args = ap.parse_args()

    import mcq_amd

    abi, quench = mcq_amd.abi, mcq_amd.quench
    rep = {"resources": resources(mcq_amd), "lds": {str(n): abi.relink3d_lds_bytes(n) for n in SHAPE_ENDS.values()}, "cases": []}
    if not args.resources_only:
        import numpy as np
        import torch

        if mcq_amd._lib.device_count() < 1:
            raise RuntimeError("relink3d_study needs a GPU (or --resources-only)")
        sp = {"type": "linear_annealing", "beta_start": 1.0, "beta_end": 3.0}
        dev = torch.device("cuda", torch.cuda.current_device())
        n = args.chains
        seeds = abi.seeds_for(42, n)
        dseeds = torch.from_numpy(np.ascontiguousarray(seeds, dtype=np.uint32).view(np.int32)).to(dev)
        rep.update(chains=n, sweeps=args.sweeps, tabu_iters=args.tabu_iters, board_hops=args.board_hops, reps=args.reps, inner=args.inner, time_iters=args.time_iters,
                   device=f"{torch.cuda.get_device_name(dev)} ({torch.cuda.get_device_properties(dev).gcnArchName})")
        for N in args.Ns:
            case = {"N": N}
            res = mcq_amd.heatbath.anneal_heatbath(N, args.sweeps, "random", sp, seeds, mcmc_type="full_3d")
            walked = quench.tabu_queens(N, res["best_state"], seeds, args.tabu_iters, tenure=10, tenure_rand=10)
            case["cube"] = dict(report(mcq_amd, torch, N, torch.from_numpy(walked["best_state"]).to(dev), dseeds, args),
                                what=f"full_3d heat bath, {args.sweeps} sweeps, then {args.tabu_iters} tabu iterations: best {int(walked['best_energy'].min())}")
            print(json.dumps({"N": N, "cube": case["cube"]}), flush=True)
            if not args.no_plateau:
                sweeps, every = SWEEPS.get(N, (500, 5))
                res, _ = mcq_amd.heatbath.anneal_heatbath(N, sweeps, "random", sp, seeds, resample_every=every)
                hopped = quench.hop_states(N, res["best_state"], seeds, args.board_hops, kick=2, local_search="pairs")
                plateau = quench.quench_queens(N, quench.queens_of_boards(N, hopped["best_state"]), conflicts=False)
                case["plateau"] = dict(report(mcq_amd, torch, N, torch.from_numpy(plateau["state"]).to(dev), dseeds, args),
                                       what=f"board heat bath, {sweeps} sweeps resampled every {every}, then {args.board_hops} board hops (pairs, kick 2), carried into the "
                                            f"cube and quenched there: board best {int(hopped['best_energy'].min())}, in the cube {int(plateau['energy_out'].min())}")
                print(json.dumps({"N": N, "plateau": case["plateau"]}), flush=True)
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
