#!/usr/bin/env python3
"""What basin hopping finds below full_3d minima, whether board plateaus fall once the queens may leave their columns, and what a hop
costs, on one MI355X (profiles/hops3d.md).

    python tools/hop3d_study.py [--chains 4096] [--Ns 12 15] [--hops 1000] [--time-hops 20] [--out FILE.json] [--profile profiles/hops3d.md]
    python tools/hop3d_study.py --resources [--profile profiles/hops3d.md]      (no GPU: the compiler's resource table only)

Random init, linear 1 -> 3, seeds 42 + r, no trace.  Per N two sets of placements go through hop_queens_device, --hops hops, slack 0, for
kick in {1, 2, 4, N}:
  (a) best_state of the full_3d heat bath (--sweeps queen sweeps, Q = N^2);
  (b) the board plateau: best_state of the board heat bath resampled as population annealing does (700 sweeps every 7 at N = 12, 445
      every 4 at N = 15) behind --board-hops board hops with the pair-move search (hop_device, kick 2), carried into the cube by
      queens_of_boards.  energy_in of the cube run is the board's energy: the question is how far best_energy falls below it.
Recorded per case: min / p10 / median of energy_in, energy_start and best_energy; accepted / hops; n_improved; the share of chains
improved; moves, passes and moved draws per hop; and the invariants -- best_energy is the first minimum of energy_hist, the history
never rises, quench_queens_device moves nothing on state and best_state and recounts their energies.
  (c) for kick = 2 on the placements of (a), milliseconds of ONE call of --time-hops hops by HIP events (best of --reps after a warm-up)
      and, in the same process on the same placements, the same work composed from the calls the library had before: per hop a kick on
      torch tensors (a random queen to a random cell where that is free), quench_queens_device, and torch.where on the energies.  The
      composed form draws from torch's generator, so it walks other minima: the same work, not the same run.
With --profile the sections between the `study` and the `resources` markers of that file are replaced."""
import argparse
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BEGIN, END = "<!-- study:begin -->", "<!-- study:end -->"
RBEGIN, REND = "<!-- resources:begin -->", "<!-- resources:end -->"
SWEEPS = {12: (700, 7), 15: (445, 4)}


def quantiles(e):
    import numpy as np

    return {"min": int(e.min()), "p10": float(np.percentile(e, 10)), "median": float(np.median(e)), "mean": float(e.mean())}


def resources():
    """VGPRs, SGPRs, scratch, static LDS and occupancy of the three instantiations, from the compiler's remarks; needs hipcc, no GPU."""
    from importlib import import_module

    b = import_module("mcq_amd").build
    cmd = [b.hipcc(), "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++17", "--cuda-device-only", "-c", "-Rpass-analysis=kernel-resource-usage",
           "-o", os.devnull, b.HOP3D_SOURCES[0]]
    err = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    rows, cur = [], None
    for line in err.splitlines():
        m = re.search(r"remark: (.*)", line)
        if not m:
            continue
        text = m.group(1).split("[-Rpass")[0].strip()
        if text.startswith("Function Name:"):
            name = subprocess.run(["c++filt", text.split(":", 1)[1].strip()], capture_output=True, text=True).stdout.strip()
            cur = {"name": re.sub(r"^void \(anonymous namespace\)::|\(.*$", "", name)}
            rows.append(cur)
        elif cur is not None and ":" in text:
            k, v = text.split(":", 1)
            cur[k.strip()] = v.strip()
    return rows


def resources_markdown(rows):
    from importlib import import_module

    abi = import_module("mcq_amd").abi
    lines = ["`-Rpass-analysis=kernel-resource-usage`, gfx950, the three instantiations of `mcq_hop3d_kernel<W, BITS, STEPS>`; the chain's LDS is dynamic "
             "(`abi.hop3d_lds_bytes`) on top of the static bytes listed.", "",
             "| kernel | VGPRs | AGPRs | SGPRs | scratch bytes per lane | occupancy (wavefronts per SIMD) | static LDS bytes | dynamic LDS at Q = N² |", "|---|---|---|---|---|---|---|---|"]
    ends = {"64": 12, "256": 19, "1024": 32}
    for r in rows:
        w = re.search(r"<(\d+)", r["name"])
        n = ends.get(w.group(1)) if w else None
        lds = f"{abi.hop3d_lds_bytes(n)} at N = {n}" if n else ""
        lines.append(f"| `{r['name']}` | {r.get('VGPRs', '?')} | {r.get('AGPRs', '?')} | {r.get('TotalSGPRs', '?')} | {r.get('ScratchSize [bytes/lane]', '?')} | "
                     f"{r.get('Occupancy [waves/SIMD]', '?')} | {r.get('LDS Size [bytes/block]', '?')} | {lds} |")
    return "\n".join(lines)


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
    """The same work from the calls the library had before mcq_hop3d: a launch, a kick on torch tensors and a select per hop."""
    quench = mcq_amd.quench
    n, Q = states.shape[0], states.shape[1] // 3
    first = quench.quench_queens_device(N, states, conflicts=False)
    cur, E = first["state"], first["energy_out"]
    rows = torch.arange(n, device=states.device)
    for _ in range(hops):
        z = cur.reshape(n, Q, 3).clone()
        for _ in range(kick):
            q = torch.randint(0, Q, (n,), device=states.device, generator=gen)
            t = torch.randint(0, N, (n, 3), device=states.device, generator=gen).to(torch.uint8)
            free = ~(z == t[:, None, :]).all(dim=2).any(dim=1)
            z[rows, q] = torch.where(free[:, None], t, z[rows, q])
        r = quench.quench_queens_device(N, z.reshape(n, 3 * Q), conflicts=False)
        keep = r["energy_out"] <= E + slack
        cur, E = torch.where(keep[:, None], r["state"], cur), torch.where(keep, r["energy_out"], E)
    return cur, E


def hop_case(mcq_amd, torch, N, states, seeds, hops, kick):
    import numpy as np

    quench = mcq_amd.quench
    st = torch.cuda.current_stream()
    res = quench.hop_queens_device(N, states, seeds, hops, kick=kick, slack=0, hist=True)
    on_state = quench.quench_queens_device(N, res["state"], conflicts=False)
    on_best = quench.quench_queens_device(N, res["best_state"], conflicts=False)
    st.synchronize()
    got, on_state, on_best = quench.to_numpy(res), quench.to_numpy(on_state), quench.to_numpy(on_best)
    hist = got["energy_hist"].astype(np.int64)
    fixed = lambda q, e: bool(not q["n_moves"].any() and np.array_equal(q["energy_in"], e))  # noqa: E731
    per = float(max(hops, 1) * len(hist))
    return {"kick": kick, "hops": hops, "energy_in": quantiles(got["energy_in"]), "energy_start": quantiles(got["energy_start"]),
            "best_energy": quantiles(got["best_energy"]), "energy_out": quantiles(got["energy_out"]),
            "accepted_share": float(got["n_accepted"].sum()) / per, "n_improved": int(got["n_improved"].sum()),
            "chains_improved_share": float((got["best_energy"] < got["energy_start"]).mean()),
            "chains_below_input_share": float((got["best_energy"] < got["energy_in"]).mean()),
            "moves_per_hop": float(got["n_moves"].sum()) / per, "passes_per_hop": float(got["n_passes"].sum()) / per, "kicked_per_hop": float(got["n_kicked"].sum()) / per,
            "flagged": int((got["flags"] != 0).sum()),
            "checks": {"best_is_min_of_hist": bool(np.array_equal(got["best_energy"], hist.min(axis=1)) and np.array_equal(got["best_hop"], hist.argmin(axis=1))),
                       "hist_never_rises": bool((np.diff(hist, axis=1) <= 0).all()),
                       "state_is_fixed_point": fixed(on_state, got["energy_out"]), "best_state_is_fixed_point": fixed(on_best, got["best_energy"])}}


def timing(mcq_amd, torch, N, states, seeds, args):
    st = torch.cuda.current_stream()
    quench = mcq_amd.quench
    k = args.time_hops
    gen = torch.Generator(device=states.device)
    gen.manual_seed(1)
    one_ms, one_all = timed(torch, st, args.reps, lambda: quench.hop_queens_device(N, states, seeds, k, kick=2, slack=0, stream=st))
    comp_ms, comp_all = timed(torch, st, args.reps, lambda: composed(mcq_amd, torch, N, states, k, 2, 0, gen))
    zero_ms, _ = timed(torch, st, args.reps, lambda: quench.hop_queens_device(N, states, seeds, 0, kick=2, slack=0, stream=st))
    return {"time_hops": k, "hop_ms": one_ms, "hop_ms_all": one_all, "composed_ms": comp_ms, "composed_ms_all": comp_all, "no_hops_ms": zero_ms,
            "hop_ms_per_hop": (one_ms - zero_ms) / k, "composed_ms_per_hop": comp_ms / k, "ratio": one_ms / comp_ms}


def markdown(rep):
    q = lambda d: f"{d['min']} / {d['p10']:g} / {d['median']:g}"  # noqa: E731
    lines = [f"Measured by `tools/hop3d_study.py` in one session on one {rep['device']}: {rep['chains']} chains, linear 1 → 3, seeds 42 + r; the placements through "
             f"`hop_queens_device`, {rep['hops']} hops, slack 0.", "",
             "| N | placements from | kick | `energy_in` min / p10 / median | `energy_start` min / p10 / median | `best_energy` min / p10 / median | accepted / hops | `n_improved` (all chains) | "
             "share of chains below `energy_start` | below `energy_in` | moves / passes / moved draws per hop |", "|---|---|---|---|---|---|---|---|---|---|---|"]
    for case in rep["cases"]:
        for name in ("cube", "plateau"):
            for r in case[name]["rows"]:
                lines.append(f"| {case['N']} | {case[name]['what']} | {r['kick']} | {q(r['energy_in'])} | {q(r['energy_start'])} | {q(r['best_energy'])} | {r['accepted_share']:.3f} | "
                             f"{r['n_improved']} | {r['chains_improved_share']:.4f} | {r['chains_below_input_share']:.4f} | "
                             f"{r['moves_per_hop']:.2f} / {r['passes_per_hop']:.2f} / {r['kicked_per_hop']:.2f} |")
    ok = all(all(r["checks"].values()) and r["flagged"] == 0 for case in rep["cases"] for n in ("cube", "plateau") for r in case[n]["rows"])
    lines += ["", "In every case `best_energy` / `best_hop` are the first minimum of `energy_hist`, the history never rises, no placement is flagged, and `quench_queens_device` moves "
              "nothing on any `state` or `best_state` and recounts the energies reported." if ok else "NOT every case passed the invariants: see the JSON.", "",
              f"Time of one call of {rep['time_hops']} hops (kick 2) on the placements of the full_3d heat bath, HIP events, best of {rep['reps']} after a warm-up call, against the "
              "composed calls (per hop a kick on torch tensors, `quench_queens_device`, `torch.where`) in the same process on the same placements. The composed form draws its kicks "
              "from torch's generator: the same work, not the same run.", "",
              "| N | `hop_queens_device` ms | of which the first descent (a call of 0 hops) | ms per hop | composed ms | composed ms per hop | ratio single launch / composed |",
              "|---|---|---|---|---|---|---|"]
    for case in rep["cases"]:
        t = case["timing"]
        lines.append(f"| {case['N']} | {t['hop_ms']:.2f} | {t['no_hops_ms']:.2f} | {t['hop_ms_per_hop']:.3f} | {t['composed_ms']:.2f} | {t['composed_ms_per_hop']:.3f} | {t['ratio']:.2f} |")
    slower = [case["N"] for case in rep["cases"] if case["timing"]["ratio"] >= 1]
    lines += ["", ("The single launch is the faster of the two at every N measured." if not slower else
                   f"The single launch is NOT the faster of the two at N = {', '.join(map(str, slower))}.")]
    return "\n".join(lines)


def splice(path, begin, end, body):
    with open(path) as f:
        text = f.read()
    if begin not in text or end not in text:
        raise RuntimeError(f"{path} has no {begin} markers")
    with open(path, "w") as f:
        f.write(text[: text.index(begin) + len(begin)] + "\n" + body + "\n" + text[text.index(end):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=4096)
    ap.add_argument("--Ns", type=int, nargs="+", default=[12, 15])
    ap.add_argument("--sweeps", type=int, default=200)
    ap.add_argument("--board-hops", type=int, default=1000)
    ap.add_argument("--hops", type=int, default=1000)
    ap.add_argument("--time-hops", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile", default=None)
    args = ap.parse_args()

    if args.resources:
        rows = resources()
        print(resources_markdown(rows))
        if args.profile:
            splice(args.profile, RBEGIN, REND, resources_markdown(rows))
        return

    import numpy as np
    import torch

    import mcq_amd

    abi, quench = mcq_amd.abi, mcq_amd.quench
    if mcq_amd._lib.device_count() < 1:
        raise RuntimeError("hop3d_study needs a GPU (--resources does not)")
    sp = {"type": "linear_annealing", "beta_start": 1.0, "beta_end": 3.0}
    dev = torch.device("cuda", torch.cuda.current_device())
    n = args.chains
    seeds = abi.seeds_for(42, n)
    dseeds = torch.from_numpy(np.ascontiguousarray(seeds, dtype=np.uint32).view(np.int32)).to(dev)
    rep = {"chains": n, "sweeps": args.sweeps, "board_hops": args.board_hops, "hops": args.hops, "time_hops": args.time_hops, "reps": args.reps,
           "device": torch.cuda.get_device_name(dev), "cases": []}
    for N in args.Ns:
        case = {"N": N}
        res = mcq_amd.heatbath.anneal_heatbath(N, args.sweeps, "random", sp, seeds, mcmc_type="full_3d")
        cube = torch.from_numpy(res["best_state"]).to(dev)
        case["cube"] = {"what": f"full_3d heat bath, {args.sweeps} sweeps", "rows": [hop_case(mcq_amd, torch, N, cube, dseeds, args.hops, k) for k in (1, 2, 4, N)]}
        print(json.dumps({"N": N, "cube": case["cube"]}), flush=True)
        sweeps, every = SWEEPS.get(N, (500, 5))
        res, _ = mcq_amd.heatbath.anneal_heatbath(N, sweeps, "random", sp, seeds, resample_every=every)
        hopped = quench.hop_states(N, res["best_state"], seeds, args.board_hops, kick=2, local_search="pairs")
        plateau = torch.from_numpy(quench.queens_of_boards(N, hopped["best_state"])).to(dev)
        case["plateau"] = {"what": f"board heat bath, {sweeps} sweeps resampled every {every}, then {args.board_hops} board hops (pairs, kick 2): "
                                   f"board best {int(hopped['best_energy'].min())}",
                           "board_best_energy": quantiles(hopped["best_energy"]),
                           "rows": [hop_case(mcq_amd, torch, N, plateau, dseeds, args.hops, k) for k in (1, 2, 4, N)]}
        print(json.dumps({"N": N, "plateau": case["plateau"]}), flush=True)
        case["timing"] = timing(mcq_amd, torch, N, cube, dseeds, args)
        print(json.dumps({"N": N, "timing": case["timing"]}), flush=True)
        rep["cases"].append(case)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rep, f, indent=1)
    if args.profile:
        splice(args.profile, BEGIN, END, markdown(rep))


if __name__ == "__main__":
    main()
