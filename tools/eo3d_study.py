#!/usr/bin/env python3
"""What extremal optimisation does on the plateaus of the cube, and what an iteration costs next to a full_3d tabu iteration, on one
MI355X (profiles/eo3d.md).

    python tools/eo3d_study.py [--chains 4096] [--Ns 12 15] [--iters 1000 10000] [--out FILE.json] [--profile profiles/eo3d.md]
    python tools/eo3d_study.py --resources-only [--profile profiles/eo3d.md]      (no GPU: the compiler's resource table only)
    python tools/eo3d_study.py --from-json FILE.json --profile profiles/eo3d.md   (no GPU: the tables of a stored report)

The placements of tools/tabu3d_study.py (profiles/tabu3d.md): random init, linear 1 -> 3, seeds 42 + r, no trace, Q = N^2.  Per N
  (a) best_state of the full_3d heat bath (--sweeps queen sweeps), and
  (b) the board plateau: best_state of the board heat bath resampled as population annealing does (700 sweeps every 7 at N = 12, 445
      every 4 at N = 15) behind --board-hops board hops with the pair-move search, carried into the cube by queens_of_boards
go through eo_queens_device for each of --iters iterations, each tau of TAUS and both moves.  Recorded per case, in ONE process:
  - milliseconds per iteration of eo_queens_device (tau = 1.4, both moves) and of tabu_queens_device (tenure 10 + (0 .. 10)) on the same
    placements: HIP events around one call of --time-iters iterations, best of --reps after a warm-up, less a call of 0 iterations; and
    their ratio, whatever it is;
  - min / 10th percentile / median of best_energy per (iterations, tau, move), and of tabu_queens_device at the same iteration counts;
  - the same for as many EO iterations as fit the launch time of tabu's iteration counts ("equal launch time");
  - the invariants: quench_queens_device recounts best_energy on best_state, moves and idle iterations add up to the iterations, and no
    placement is flagged.
It also records the compiler's resource table of the three instantiations of the kernel (VGPRs, SGPRs, spills, scratch) from a compile
of csrc/mcq_eo3d.hip with -Rpass-analysis=kernel-resource-usage; that part needs no GPU.
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
TAUS = (1.2, 1.4, 1.6, 2.0, float("inf"))
TABU = dict(tenure=10, tenure_rand=10)
SHAPE_ENDS = {64: 12, 256: 19, 1024: 32}  # lanes per chain -> the largest N of the instantiation


def resources(mcq_amd):
    """{W: {vgprs, sgprs, lds, scratch, occupancy, spills}} from the compiler's remarks."""
    b = mcq_amd.build
    cmd = [b.hipcc()] + [f for f in b.FLAGS if f != "-shared"] + ["-c", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-o", os.devnull, b.EO3D_SOURCES[0]]
    err = subprocess.run(cmd, capture_output=True, text=True).stderr
    out, cur = {}, None
    for line in err.splitlines():
        m = re.search(r"Function Name: \S*mcq_eo3d_kernelILi(\d+)E", line)
        if m:
            cur = out.setdefault(int(m.group(1)), {})
        for key, pat in (("vgprs", r" VGPRs: (\d+)"), ("sgprs", r"TotalSGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)"),
                         ("vgpr_spills", r"VGPRs Spill: (\d+)"), ("sgpr_spills", r"SGPRs Spill: (\d+)")):
            m = re.search(pat, line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    return out


def quantiles(e):
    import numpy as np

    return {"min": int(e.min()), "p10": float(np.percentile(e, 10)), "median": float(np.median(e))}


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

    eo, quench = mcq_amd.eo, mcq_amd.quench
    st = torch.cuda.current_stream()
    dev = states.device
    tables = {tau: torch.from_numpy(eo.rank_table(N, tau, N * N).view(np.int32)).to(dev) for tau in TAUS}
    T = args.time_iters
    tabu0 = timed(torch, st, args.reps, lambda: quench.tabu_queens_device(N, states, seeds, 0, stream=st))
    tabu_ms = (timed(torch, st, args.reps, lambda: quench.tabu_queens_device(N, states, seeds, T, stream=st, **TABU)) - tabu0) / T
    eo0 = timed(torch, st, args.reps, lambda: eo.eo_queens_device(N, states, seeds, 0, rank_cdf=tables[1.4], stream=st))
    eo_ms = {mv: (timed(torch, st, args.reps, lambda: eo.eo_queens_device(N, states, seeds, T, rank_cdf=tables[1.4], move=mv, stream=st)) - eo0) / T for mv in eo.MOVES}
    out = {"tabu_ms_per_iter": tabu_ms, "eo_ms_per_iter": eo_ms, "ratio": {mv: eo_ms[mv] / tabu_ms for mv in eo.MOVES}, "tabu_no_iters_ms": tabu0, "eo_no_iters_ms": eo0,
           "time_iters": T, "rows": [], "tabu_rows": []}
    print(f"N={N}: tabu {tabu_ms:.5f} ms per iteration, EO {eo_ms}", file=sys.stderr, flush=True)
    for iters in args.iters:
        t = quench.tabu_queens_device(N, states, seeds, iters, **TABU)
        st.synchronize()
        t = quench.tabu_to_numpy(t)
        out["tabu_rows"].append({"iters": iters, "energy_in": quantiles(t["energy_in"]), "best_energy": quantiles(t["best_energy"]), "launch_ms": tabu0 + iters * tabu_ms})
        for mv in eo.MOVES:
            equal = max(1, int(round(iters * tabu_ms / max(eo_ms[mv], 1e-9))))  # the EO iterations that fit tabu's launch
            for tau in TAUS:
                for n_iters, kind in ((iters, "same iterations"), (equal, "equal launch time")):
                    res = eo.eo_queens_device(N, states, seeds, n_iters, rank_cdf=tables[tau], move=mv)
                    on_best = quench.quench_queens_device(N, res["best_state"], conflicts=False)
                    st.synchronize()
                    got, on_best = eo.to_numpy(res), quench.to_numpy(on_best)
                    per = float(n_iters * len(got["n_moves"]))
                    checks = {"best_state_recounts": bool(np.array_equal(on_best["energy_in"], got["best_energy"])),
                              "moves_and_idle_add_up": bool((got["n_moves"] + got["n_idle"] == n_iters).all()), "none_flagged": bool(not got["flags"].any())}
                    out["rows"].append({"tabu_iters": iters, "kind": kind, "iters": n_iters, "tau": tau, "move": mv, "energy_in": quantiles(got["energy_in"]),
                                        "best_energy": quantiles(got["best_energy"]), "energy_out": quantiles(got["energy_out"]),
                                        "below_start_share": float((got["best_energy"] < got["energy_in"]).mean()), "uphill": got["n_uphill"].sum() / per,
                                        "flat": got["n_flat"].sum() / per, "free": got["n_free"].sum() / per, "idle": got["n_idle"].sum() / per, "checks": checks})
                    print(f"N={N} {kind} {n_iters} {mv} tau={tau}: best {out['rows'][-1]['best_energy']}", file=sys.stderr, flush=True)
    return out


def markdown(rep):
    q = lambda d: f"{d['min']} / {d['p10']:g} / {d['median']:g}"  # noqa: E731
    tau = lambda t: "∞" if t == float("inf") else f"{t:g}"  # noqa: E731
    lines = ["Compiler's resource table of `csrc/mcq_eo3d.hip` (`-Rpass-analysis=kernel-resource-usage`, gfx950), the three instantiations of "
             "`mcq_eo3d_kernel<W, BITS, STEPS>`; the chain's LDS is dynamic (`abi.eo3d_lds_bytes`) on top of the static bytes listed:", "",
             "| lanes per chain W | VGPRs | SGPRs | VGPRs spilled | SGPRs spilled (to VGPR lanes) | static LDS bytes | scratch bytes per lane | waves per SIMD | dynamic LDS at Q = N² "
             "| at Q = N³ − 1 |", "|---|---|---|---|---|---|---|---|---|---|"]
    for W, r in sorted(rep["resources"].items(), key=lambda kv: int(kv[0])):
        n = SHAPE_ENDS.get(int(W))
        lines.append(f"| {W} | {r.get('vgprs')} | {r.get('sgprs')} | {r.get('vgpr_spills')} | {r.get('sgpr_spills')} | {r.get('lds')} | {r.get('scratch')} | {r.get('occupancy')} | "
                     f"{rep['lds'].get(str(n), ['', ''])[0]} at N = {n} | {rep['lds'].get(str(n), ['', ''])[1]} |")
    clean = not any(r.get("scratch") or r.get("vgpr_spills") for r in rep["resources"].values())
    lines += ["", "No instantiation uses scratch or spills a VGPR." if clean else "Some instantiations use scratch or spill VGPRs: see the table."]
    if not rep.get("cases"):
        return "\n".join(lines + ["", "Not measured: no GPU session was had for the figures below the resource table.  No time per iteration and no energy of "
                                  "`eo_queens_device` is on record."])
    lines += ["", f"Measured by `tools/eo3d_study.py` in one process on one {rep['device']}: {rep['chains']} chains of N² queens, linear 1 → 3, seeds 42 + r; the placements through "
              f"`eo_queens_device` and `tabu_queens_device` (tenure 10 + (0 … 10)). Times are HIP events around one call of {rep['time_iters']} iterations, best of {rep['reps']} after "
              "a warm-up, less a call of 0 iterations.", "",
              "| N | placements from | tabu ms per iteration | EO ms per iteration, best / random | EO / tabu, best / random |", "|---|---|---|---|---|"]
    for case in rep["cases"]:
        for name in ("cube", "plateau"):
            c = case[name]
            lines.append(f"| {case['N']} | {c['what']} | {c['tabu_ms_per_iter']:.4f} | {c['eo_ms_per_iter']['best']:.4f} / {c['eo_ms_per_iter']['random']:.4f} | "
                         f"{c['ratio']['best']:.3f} / {c['ratio']['random']:.3f} |")
    lines += ["", "`best_energy` as min / 10th percentile / median over the chains. \"equal launch time\" runs as many EO iterations as fit the launch of that many tabu iterations:", "",
              "| N | placements from | `energy_in` | tabu iterations | tabu `best_energy` | move | τ | EO `best_energy`, same iterations | EO iterations in equal launch time | EO `best_energy`, equal "
              "launch time | share of chains below their start (equal time) | uphill / flat / free moves per iteration (equal time) |", "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    ok = True
    for case in rep["cases"]:
        for name in ("cube", "plateau"):
            c = case[name]
            for t in c["tabu_rows"]:
                rows = [r for r in c["rows"] if r["tabu_iters"] == t["iters"]]
                for same in (r for r in rows if r["kind"] == "same iterations"):
                    eq = next(r for r in rows if r["kind"] == "equal launch time" and r["tau"] == same["tau"] and r["move"] == same["move"])
                    ok = ok and all(same["checks"].values()) and all(eq["checks"].values())
                    lines.append(f"| {case['N']} | {c['what']} | {q(t['energy_in'])} | {t['iters']} | {q(t['best_energy'])} | {same['move']} | {tau(same['tau'])} | {q(same['best_energy'])} | "
                                 f"{eq['iters']} | {q(eq['best_energy'])} | {eq['below_start_share']:.4f} | {eq['uphill']:.3f} / {eq['flat']:.3f} / {eq['free']:.4f} |")
    lines += ["", "In every case `quench_queens_device` recounts `best_energy` on `best_state`, moves and idle iterations add up to the iterations, and no placement is flagged."
              if ok else "NOT every case passed the invariants: see the JSON."]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=4096)
    ap.add_argument("--Ns", type=int, nargs="+", default=[12, 15])
    ap.add_argument("--sweeps", type=int, default=200)
    ap.add_argument("--board-hops", type=int, default=1000)
    ap.add_argument("--iters", type=int, nargs="+", default=[1000, 10000])
    ap.add_argument("--time-iters", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--resources-only", action="store_true")
    ap.add_argument("--from-json", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile", default=None)
    args = ap.parse_args()

    import mcq_amd

    abi, quench = mcq_amd.abi, mcq_amd.quench
    if args.from_json:
        with open(args.from_json) as f:
            rep = json.load(f)
        for case in rep["cases"]:  # (JSON has no infinity of its own that every reader takes: it is stored as a string)
            for name in ("cube", "plateau"):
                for r in case[name]["rows"]:
                    r["tau"] = float(r["tau"])
    else:
        rep = {"resources": resources(mcq_amd), "lds": {str(n): [abi.eo3d_lds_bytes(n), abi.eo3d_lds_bytes(n, n ** 3 - 1)] for n in SHAPE_ENDS.values()}, "cases": []}
    if not args.resources_only and not args.from_json:
        import numpy as np
        import torch

        if mcq_amd._lib.device_count() < 1:
            raise RuntimeError("eo3d_study needs a GPU (or --resources-only)")
        sp = {"type": "linear_annealing", "beta_start": 1.0, "beta_end": 3.0}
        dev = torch.device("cuda", torch.cuda.current_device())
        n = args.chains
        seeds = abi.seeds_for(42, n)
        dseeds = torch.from_numpy(np.ascontiguousarray(seeds, dtype=np.uint32).view(np.int32)).to(dev)
        rep.update(chains=n, sweeps=args.sweeps, board_hops=args.board_hops, reps=args.reps, time_iters=args.time_iters,
                   device=f"{torch.cuda.get_device_name(dev)} ({torch.cuda.get_device_properties(dev).gcnArchName})")
        for N in args.Ns:
            case = {"N": N}
            res = mcq_amd.heatbath.anneal_heatbath(N, args.sweeps, "random", sp, seeds, mcmc_type="full_3d")
            case["cube"] = dict(report(mcq_amd, torch, N, torch.from_numpy(res["best_state"]).to(dev), dseeds, args), what=f"full_3d heat bath, {args.sweeps} sweeps")
            sweeps, every = SWEEPS.get(N, (500, 5))
            res, _ = mcq_amd.heatbath.anneal_heatbath(N, sweeps, "random", sp, seeds, resample_every=every)
            hopped = quench.hop_states(N, res["best_state"], seeds, args.board_hops, kick=2, local_search="pairs")
            plateau = torch.from_numpy(quench.queens_of_boards(N, hopped["best_state"])).to(dev)
            case["plateau"] = dict(report(mcq_amd, torch, N, plateau, dseeds, args),
                                   what=f"board heat bath, {sweeps} sweeps resampled every {every}, then {args.board_hops} board hops (pairs, kick 2): "
                                        f"board best {int(hopped['best_energy'].min())}")
            rep["cases"].append(case)
            if args.out:  # (what is measured so far is kept, case by case)
                dump(rep, args.out)
    if args.out and not args.from_json:
        dump(rep, args.out)
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


def dump(rep, path):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    stored = json.loads(json.dumps(rep).replace("Infinity", '"inf"'))
    with open(path, "w") as f:
        json.dump(stored, f, indent=1)


if __name__ == "__main__":
    main()
