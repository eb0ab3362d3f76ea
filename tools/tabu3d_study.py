#!/usr/bin/env python3
"""Whether tabu search goes below what the full_3d hops reach, and what an iteration costs next to a hop, on one MI355X
(profiles/tabu3d.md).

    python tools/tabu3d_study.py [--chains 4096] [--Ns 12 15] [--iters 1000 10000] [--test-log FILE] [--out FILE.json] [--profile profiles/tabu3d.md]
    python tools/tabu3d_study.py --resources-only [--profile profiles/tabu3d.md]      (no GPU: the compiler's resource table only)

The setup of tools/hop3d_study.py: random init, linear 1 -> 3, seeds 42 + r, no trace, Q = N^2.  Per N two sets of placements go
through tabu_queens_device for each of --iters iterations and each tenure of TENURES (those of tools/tabu_study.py):
  (a) best_state of the full_3d heat bath (--sweeps queen sweeps);
  (b) the board plateau: best_state of the board heat bath resampled as population annealing does (700 sweeps every 7 at N = 12, 445
      every 4 at N = 15) behind --board-hops board hops with the pair-move search, carried into the cube by queens_of_boards.
Recorded per case:
  - milliseconds of the call by HIP events (best of --reps after a warm-up), less a call of 0 iterations, per iteration;
  - min / median of energy_in and of best_energy, the share of chains below their start, the four counters per iteration;
  - next to it hop_queens_device (kick 2, slack 0) on the same placements with as many hops as take the same launch time, from its own
    time per hop measured in the same session;
  - milliseconds per iteration for 1, 3 and 64 chains in each shape of the kernel (N = 12, 19, 32);
  - with --test-log, the wall time of each test of tests/test_tabu3d.py from a `pytest --durations=0` log.
It also records the compiler's resource table of the three instantiations (VGPRs, SGPRs, scratch, static LDS, waves per SIMD) from a
compile of csrc/mcq_tabu3d.hip with -Rpass-analysis=kernel-resource-usage; that part needs no GPU.
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
TENURES = ((2, 0, 0), (5, 5, 0), (10, 10, 0), (0, 9, 10), (40, 20, 0))  # (tenure, tenure_rand, tenure_conf), as in tools/tabu_study.py
SHAPE_ENDS = {64: 12, 256: 19, 1024: 32}  # lanes per chain -> the largest N of the instantiation


def resources(mcq_amd):
    """{W: {vgprs, sgprs, lds, scratch, occupancy}} from the compiler's remarks."""
    b = mcq_amd.build
    cmd = [b.hipcc()] + [f for f in b.FLAGS if f != "-shared"] + ["-c", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-o", os.devnull, b.TABU3D_SOURCES[0]]
    err = subprocess.run(cmd, capture_output=True, text=True).stderr
    out, cur = {}, None
    for line in err.splitlines():
        m = re.search(r"Function Name: \S*mcq_tabu3d_kernelILi(\d+)E", line)
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
    """(best milliseconds of `reps` calls behind a warm-up, the result of the last call)."""
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
    return min(ms), res


def report(mcq_amd, torch, N, states, seeds, args):
    import numpy as np

    quench = mcq_amd.quench
    st = torch.cuda.current_stream()
    zero_ms, _ = timed(torch, st, args.reps, lambda: quench.tabu_queens_device(N, states, seeds, 0, stream=st))
    hop0_ms, _ = timed(torch, st, args.reps, lambda: quench.hop_queens_device(N, states, seeds, 0, stream=st))
    hop_ms = (timed(torch, st, args.reps, lambda: quench.hop_queens_device(N, states, seeds, args.time_hops, kick=2, stream=st))[0] - hop0_ms) / args.time_hops
    rows = []
    for iters in args.iters:
        for tenure, rand, conf in TENURES:
            kw = dict(tenure=tenure, tenure_rand=rand, tenure_conf=conf)
            ms, res = timed(torch, st, args.reps, lambda: quench.tabu_queens_device(N, states, seeds, iters, stream=st, **kw))
            on_best = quench.quench_queens_device(N, res["best_state"], conflicts=False)
            st.synchronize()
            got, on_best = quench.tabu_to_numpy(res), quench.to_numpy(on_best)
            applies = got["best_iter"] < iters
            checks = {"best_state_recounts": bool(np.array_equal(on_best["energy_in"], got["best_energy"])),
                      "best_state_is_minimum": bool(not on_best["n_moves"][applies].any()),
                      "moves_and_stalls_add_up": bool((got["n_moves"] + got["n_stalled"] == iters).all()), "none_flagged": bool(not got["flags"].any())}
            per = float(iters * len(got["n_moves"]))
            rows.append({"iters": iters, "tenure": tenure, "tenure_rand": rand, "tenure_conf": conf, "ms": ms, "ms_per_iter": (ms - zero_ms) / iters,
                         "energy_in": quantiles(got["energy_in"]), "best_energy": quantiles(got["best_energy"]), "energy_out": quantiles(got["energy_out"]),
                         "below_start_share": float((got["best_energy"] < got["energy_in"]).mean()), "moves": got["n_moves"].sum() / per,
                         "uphill": got["n_uphill"].sum() / per, "aspired": got["n_aspired"].sum() / per, "stalled": got["n_stalled"].sum() / per, "checks": checks})
            print(f"N={N} iters={iters} tenure={tenure}+{rand}+{conf}/16 F: {ms:.1f} ms, best {rows[-1]['best_energy']['min']}", file=sys.stderr, flush=True)
        hops = max(1, int(round(min(r["ms"] for r in rows if r["iters"] == iters) / max(hop_ms, 1e-6))))
        h = quench.hop_queens_device(N, states, seeds, hops, kick=2)
        st.synchronize()
        h = quench.to_numpy(h)
        rows.append({"iters": iters, "hops": hops, "hop_energy_start": quantiles(h["energy_start"]), "hop_best_energy": quantiles(h["best_energy"]),
                     "hop_below_start_share": float((h["best_energy"] < h["energy_in"]).mean())})
    return {"rows": rows, "tabu_no_iters_ms": zero_ms, "hop_ms_per_hop": hop_ms, "hop_no_hops_ms": hop0_ms}


def few_chains(mcq_amd, torch, args):
    """Milliseconds per iteration for 1, 3 and 64 random placements of N^2 queens at the largest N of each shape: what sizes the tests."""
    import numpy as np

    quench, abi = mcq_amd.quench, mcq_amd.abi
    dev = torch.device("cuda", torch.cuda.current_device())
    st = torch.cuda.current_stream()
    rows = []
    for W, N in SHAPE_ENDS.items():
        for n in (1, 3, 64):
            rs = np.random.RandomState(N + n)
            flat = np.stack([rs.choice(N ** 3, size=N * N, replace=False) for _ in range(n)])
            s = np.stack([flat // (N * N), (flat // N) % N, flat % N], axis=2).astype(np.uint8).reshape(n, -1)
            t, sd = torch.from_numpy(s).to(dev), torch.from_numpy(abi.seeds_for(1, n).view(np.int32)).to(dev)
            zero, _ = timed(torch, st, args.reps, lambda: quench.tabu_queens_device(N, t, sd, 0, stream=st))
            ms, res = timed(torch, st, args.reps, lambda: quench.tabu_queens_device(N, t, sd, args.few_iters, tenure=10, tenure_rand=10, stream=st))
            rows.append({"W": W, "N": N, "chains": n, "iters": args.few_iters, "ms": ms, "ms_per_iter": (ms - zero) / args.few_iters,
                         "moves": float(res["n_moves"].sum().item()) / (n * args.few_iters)})
    return rows


def test_times(path):
    rows = []
    with open(path) as f:
        for line in f:
            m = re.match(r"\s*([0-9.]+)s call\s+tests/test_tabu3d.py::(\S+)", line)
            if m:
                rows.append((m.group(2), float(m.group(1))))
    return rows


def markdown(rep):
    q = lambda d: f"{d['min']} / {d['median']:g}"  # noqa: E731
    lines = ["Compiler's resource table of `csrc/mcq_tabu3d.hip` (`-Rpass-analysis=kernel-resource-usage`, gfx950), the three instantiations of "
             "`mcq_tabu3d_kernel<W, BITS, STEPS>`; the chain's LDS is dynamic (`abi.tabu3d_lds_bytes`) on top of the static bytes listed:", "",
             "| lanes per chain W | VGPRs | SGPRs | static LDS bytes | scratch bytes per lane | waves per SIMD | dynamic LDS at Q = N² |", "|---|---|---|---|---|---|---|"]
    for W, r in sorted(rep["resources"].items(), key=lambda kv: int(kv[0])):
        n = SHAPE_ENDS.get(int(W))
        lines.append(f"| {W} | {r.get('vgprs')} | {r.get('sgprs')} | {r.get('lds')} | {r.get('scratch')} | {r.get('occupancy')} | {rep['lds'].get(str(n), '')} at N = {n} |")
    spills = [W for W, r in rep["resources"].items() if r.get("scratch")]
    lines += ["", "No instantiation uses scratch." if not spills else f"Scratch is NOT 0 at W = {', '.join(map(str, spills))}."]
    if not rep.get("cases"):
        return "\n".join(lines)
    lines += ["", f"Measured by `tools/tabu3d_study.py` in one session on one {rep['device']}: {rep['chains']} chains of N² queens, linear 1 → 3, seeds 42 + r; the placements "
              f"through `tabu_queens_device`. Times are HIP events around one call, best of {rep['reps']} after a warm-up, less a call of 0 iterations.", "",
              "| N | placements from | iterations | tenure + rand + conf/16·F | ms | ms per iteration | `energy_in` min / median | `best_energy` min / median | share of chains below "
              "their start | moves / uphill / aspired / stalled per iteration |", "|---|---|---|---|---|---|---|---|---|---|"]
    hop_lines = ["", "`hop_queens_device` (kick 2, slack 0) on the same placements, with as many hops as fit the fastest tabu launch of that many iterations, from its own time per "
                 "hop in the same session:", "",
                 "| N | placements from | ms per hop | launch time of … tabu iterations | hops | `energy_start` min / median | `best_energy` min / median | share of chains below their input |",
                 "|---|---|---|---|---|---|---|---|"]
    ok = True
    for case in rep["cases"]:
        for name in ("cube", "plateau"):
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
    lines += ["", "In every case `quench_queens_device` recounts `best_energy` on `best_state` and moves nothing on a `best_state` behind which an iteration ran, moves and stalls add up "
              "to the iterations, and no placement is flagged." if ok else "NOT every case passed the invariants: see the JSON."]
    lines += ["", f"Few chains, random placements of N² queens, {rep['few'][0]['iters']} iterations with tenure 10 + (0 … 10), at the largest N of each shape (what sizes the GPU tests):", "",
              "| lanes per chain W | N | chains | ms | ms per iteration | moves per iteration |", "|---|---|---|---|---|---|"]
    for r in rep["few"]:
        lines.append(f"| {r['W']} | {r['N']} | {r['chains']} | {r['ms']:.2f} | {r['ms_per_iter']:.4f} | {r['moves']:.3f} |")
    if rep.get("tests"):
        lines += ["", "Wall time of each test of `tests/test_tabu3d.py` (pytest's `call` durations, the host code's and the restatement's share included):", "",
                  "| test | seconds |", "|---|---|"]
        lines += [f"| `{name}` | {secs:.2f} |" for name, secs in rep["tests"]]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=4096)
    ap.add_argument("--Ns", type=int, nargs="+", default=[12, 15])
    ap.add_argument("--sweeps", type=int, default=200)
    ap.add_argument("--board-hops", type=int, default=1000)
    ap.add_argument("--iters", type=int, nargs="+", default=[1000, 10000])
    ap.add_argument("--time-hops", type=int, default=20)
    ap.add_argument("--few-iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--resources-only", action="store_true")
    ap.add_argument("--test-log", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile", default=None)
    args = ap.parse_args()

    import mcq_amd

    abi, quench = mcq_amd.abi, mcq_amd.quench
    rep = {"resources": resources(mcq_amd), "lds": {str(n): abi.tabu3d_lds_bytes(n) for n in SHAPE_ENDS.values()}, "cases": []}
    if args.test_log:
        rep["tests"] = test_times(args.test_log)
    if not args.resources_only:
        import numpy as np
        import torch

        if mcq_amd._lib.device_count() < 1:
            raise RuntimeError("tabu3d_study needs a GPU (or --resources-only)")
        sp = {"type": "linear_annealing", "beta_start": 1.0, "beta_end": 3.0}
        dev = torch.device("cuda", torch.cuda.current_device())
        n = args.chains
        seeds = abi.seeds_for(42, n)
        dseeds = torch.from_numpy(np.ascontiguousarray(seeds, dtype=np.uint32).view(np.int32)).to(dev)
        rep.update(chains=n, sweeps=args.sweeps, board_hops=args.board_hops, reps=args.reps,
                   device=f"{torch.cuda.get_device_name(dev)} ({torch.cuda.get_device_properties(dev).gcnArchName})")
        rep["few"] = few_chains(mcq_amd, torch, args)
        print(json.dumps({"few": rep["few"]}), flush=True)
        for N in args.Ns:
            case = {"N": N}
            res = mcq_amd.heatbath.anneal_heatbath(N, args.sweeps, "random", sp, seeds, mcmc_type="full_3d")
            case["cube"] = dict(report(mcq_amd, torch, N, torch.from_numpy(res["best_state"]).to(dev), dseeds, args), what=f"full_3d heat bath, {args.sweeps} sweeps")
            print(json.dumps({"N": N, "cube": case["cube"]}), flush=True)
            sweeps, every = SWEEPS.get(N, (500, 5))
            res, _ = mcq_amd.heatbath.anneal_heatbath(N, sweeps, "random", sp, seeds, resample_every=every)
            hopped = quench.hop_states(N, res["best_state"], seeds, args.board_hops, kick=2, local_search="pairs")
            plateau = torch.from_numpy(quench.queens_of_boards(N, hopped["best_state"])).to(dev)
            case["plateau"] = dict(report(mcq_amd, torch, N, plateau, dseeds, args),
                                   what=f"board heat bath, {sweeps} sweeps resampled every {every}, then {args.board_hops} board hops (pairs, kick 2): "
                                        f"board best {int(hopped['best_energy'].min())}")
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
