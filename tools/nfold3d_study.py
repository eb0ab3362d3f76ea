#!/usr/bin/env python3
"""What an event of the full_3d n-fold way costs next to the full_3d Metropolis sweep, and whether a cold run moves the cube's plateau,
on one MI355X (profiles/nfold3d.md).

    python tools/nfold3d_study.py [--chains 4096] [--Ns 12 15] [--const-steps 100000] [--ramp-steps 20000] [--out FILE.json] [--profile profiles/nfold3d.md]
    python tools/nfold3d_study.py --resources-only [--profile profiles/nfold3d.md]      (no GPU: the compiler's resource table only)

Per N, Q = N^2, seeds 42 + r, both through nfold_queens_device with the "exp" clock:
  - QUENCHED placements: random placements behind quench_queens_device (single-queen minima), (a) at constant beta = 3 for
    --const-steps Metropolis steps in one segment, (b) along linear 1 -> 3 over --ramp-steps steps in --ramp-segs segments;
  - the two sets of placements tools/tabu3d_study.py starts from -- best_state of the full_3d heat bath (--sweeps queen sweeps), and the
    board plateau (the resampled board heat bath behind --board-hops board hops, carried into the cube by queens_of_boards) -- at
    constant beta = 3: whether best_energy goes below the cube's 22 (N = 12) and 99 (N = 15).
Recorded per case: milliseconds of the call by HIP events less a call of no segment (the two codes warmed up once, then alternated for
--reps rounds; best and slowest round are both recorded and the derived figures use the best), per event
(events_out summed over the chains); events per Metropolis step; min / median of energy_in and best_energy; and the YARDSTICK, the
full_3d Metropolis sweep as it stands (experiments.warm_start_chains, MT19937, no trace) on the same placements and schedule in the
same process: its kernel seconds per chain-step, and the break-even, that is the chain-steps of the sweep that one event costs -- the
n-fold way is the faster one where the sweep's acceptance rate lies below its inverse.
It also records the compiler's resource table of the three instantiations from a compile of csrc/mcq_nfold3d.hip with
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
SHAPE_ENDS = {64: 12, 256: 19, 1024: 32}  # lanes per chain -> the largest N of the instantiation
PLATEAU = {12: 22, 15: 99}  # what the full_3d searches reach (profiles/hops3d.md, profiles/tabu3d.md)
SWEEPS = {12: (700, 7), 15: (445, 4)}  # the board heat bath of tools/tabu3d_study.py: sweeps, resampled every


def resources(mcq_amd):
    """{W: {vgprs, sgprs, lds, scratch, occupancy}} from the compiler's remarks."""
    b = mcq_amd.build
    cmd = [b.hipcc()] + [f for f in b.FLAGS if f != "-shared"] + ["-c", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-o", os.devnull, b.NFOLD3D_SOURCES[0]]
    err = subprocess.run(cmd, capture_output=True, text=True).stderr
    out, cur = {}, None
    for line in err.splitlines():
        m = re.search(r"Function Name: \S*mcq_nfold3d_kernelILi(\d+)E", line)
        if m:
            cur = out.setdefault(int(m.group(1)), {})
        for key, pat in (("vgprs", r" VGPRs: (\d+)"), ("sgprs", r"TotalSGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)"), ("sgpr_spills", r"SGPRs Spill: (\d+)"),
                         ("vgpr_spills", r"VGPRs Spill: (\d+)")):
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


def case(mcq_amd, torch, N, states, seeds, betas, seg_steps, what, args):
    """One schedule (a beta per segment) on the placements `states` (NumPy): the n-fold call and the sweep next to it."""
    import numpy as np

    nfold, abi = mcq_amd.nfold, mcq_amd.abi
    dev = torch.device("cuda", torch.cuda.current_device())
    st = torch.cuda.current_stream()
    n = len(states)
    t, sd = torch.from_numpy(states).to(dev), torch.from_numpy(np.ascontiguousarray(seeds, dtype=np.uint32).view(np.int32)).to(dev)
    tabs = nfold.weight_tables(betas, abi.MAX_NFOLD3D_TABLE)
    dtab = torch.from_numpy(tabs.view(np.int32)).to(dev)
    ln2, ct = nfold.clock_tables("exp")
    clock = (ln2, torch.from_numpy(ct.view(np.int32)).to(dev))
    zero_ms, _ = timed(torch, st, args.reps, lambda: nfold.nfold_queens_device(N, t, sd, dtab[:0], seg_steps, clock=clock, stream=st))
    n_steps = seg_steps * len(betas)
    # the yardstick: the full_3d Metropolis sweep as it stands, on the same placements and schedule.  Both codes are warmed up once and then
    # ALTERNATED, --reps rounds of one n-fold call (HIP events around it) and one sweep (its own HIP events around the kernel)
    sp = {"type": "constant", "beta_const": float(betas[0])} if len(betas) == 1 else {"type": "linear_annealing", "beta_start": float(betas[0]), "beta_end": float(args.beta_end)}
    sweep = lambda: mcq_amd.experiments.warm_start_chains(N, states, seeds, n_steps, sp, mcmc_type="full_3d", trace=False, states=False)[0]  # noqa: E731
    call = lambda: nfold.nfold_queens_device(N, t, sd, dtab, seg_steps, clock=clock, stream=st)  # noqa: E731
    call(), sweep()
    st.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    all_ms, all_sweep = [], []
    for _ in range(args.reps):
        e0.record(st)
        res = call()
        e1.record(st)
        st.synchronize()
        all_ms.append(e0.elapsed_time(e1) - zero_ms)
        sw = sweep()
        all_sweep.append(1e3 * float(sw["kernel_seconds"]))
    ms, sweep_ms = min(all_ms), min(all_sweep)
    got = nfold.to_numpy(res)
    events = int(got["events_out"].sum())
    row = {"N": N, "what": what, "betas": [float(betas[0]), float(betas[-1])], "n_segs": len(betas), "steps": n_steps, "ms": ms, "ms_all": sorted(all_ms), "no_segment_ms": zero_ms,
           "events": events, "events_per_chain": events / n, "events_per_step": events / (n * float(n_steps)),
           "us_per_event": 1e3 * ms / max(events, 1), "energy_in": quantiles(got["energy_in"]), "best_energy": quantiles(got["best_energy"]),
           "energy_out": quantiles(got["energy_out"]), "uphill_share": float(got["n_uphill"].sum()) / max(events, 1), "flat_share": float(got["n_flat"].sum()) / max(events, 1),
           "below_start_share": float((got["best_energy"] < got["energy_in"]).mean()), "flagged": int(got["flags"].sum())}
    row.update(sweep_ms=sweep_ms, sweep_ms_all=sorted(all_sweep), sweep_ns_per_chain_step=1e6 * sweep_ms / (n * float(n_steps)),
               sweep_accept_rate=float(sw["n_accepted"].sum()) / (n * float(n_steps)), sweep_best_energy=quantiles(sw["best_energy"]))
    row["break_even_chain_steps"] = row["us_per_event"] * 1e3 / row["sweep_ns_per_chain_step"]
    row["nfold_ms_per_sweep_ms"] = ms / sweep_ms
    row["ratio_range"] = [min(all_ms) / max(all_sweep), max(all_ms) / min(all_sweep)]  # the slowest of one against the fastest of the other, both ways
    print(json.dumps(row), file=sys.stderr, flush=True)
    return row


def markdown(rep):
    q = lambda d: f"{d['min']} / {d['median']:g}"  # noqa: E731
    lines = ["Compiler's resource table of `csrc/mcq_nfold3d.hip` (`-Rpass-analysis=kernel-resource-usage`, gfx950), the three instantiations of "
             "`mcq_nfold3d_kernel<W, BITS, STEPS>`; the chain's LDS is dynamic (`abi.nfold3d_lds_bytes`) on top of the static bytes listed:", "",
             "| lanes per chain W | VGPRs | SGPRs | SGPRs spilled to VGPRs | VGPRs spilled | static LDS bytes | scratch bytes per lane | waves per SIMD | dynamic LDS at Q = N² |",
             "|---|---|---|---|---|---|---|---|---|"]
    for W, r in sorted(rep["resources"].items(), key=lambda kv: int(kv[0])):
        n = SHAPE_ENDS.get(int(W))
        lines.append(f"| {W} | {r.get('vgprs')} | {r.get('sgprs')} | {r.get('sgpr_spills')} | {r.get('vgpr_spills')} | {r.get('lds')} | {r.get('scratch')} | {r.get('occupancy')} | "
                     f"{rep['lds'].get(str(n), '')} at N = {n} |")
    spills = [W for W, r in rep["resources"].items() if r.get("scratch")]
    lines += ["", "No instantiation uses scratch." if not spills else f"Scratch is NOT 0 at W = {', '.join(map(str, spills))}."]
    if not rep.get("cases"):
        return "\n".join(lines)
    lines += ["", f"Measured by `tools/nfold3d_study.py` in one session on one {rep['device']}: {rep['chains']} chains of N² queens, seeds 42 + r, the `exp` clock. Times are HIP "
              f"events around one call less a call of no segment; the sweep is `experiments.warm_start_chains` (MT19937, no trace) on the same placements and schedule in the same "
              f"process, its kernel's own HIP events. Both were warmed up once and then alternated for {rep['reps']} rounds; a time is given as best (slowest) of those rounds, every "
              "figure derived from times uses the best, and the bracket behind the ratio pairs the fastest round of one code with the slowest of the other, both ways.", "",
              "| N | placements | beta | Metropolis steps | n-fold ms best (slowest) | events per chain | events per step | µs per event | sweep ms best (slowest) | sweep ns per chain-step | sweep acceptance | "
              "break-even: chain-steps per event | n-fold ms / sweep ms [range] | `energy_in` min / median | n-fold `best_energy` min / median | sweep `best_energy` min / median |",
              "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rep["cases"]:
        beta = f"{r['betas'][0]:g}" if r["n_segs"] == 1 else f"{r['betas'][0]:g} → {rep['beta_end']:g} in {r['n_segs']} segments"
        lines.append(f"| {r['N']} | {r['what']} | {beta} | {r['steps']} | {r['ms']:.1f} ({r['ms_all'][-1]:.1f}) | {r['events_per_chain']:.1f} | {r['events_per_step']:.2e} | {r['us_per_event']:.3f} | "
                     f"{r['sweep_ms']:.1f} ({r['sweep_ms_all'][-1]:.1f}) | {r['sweep_ns_per_chain_step']:.3f} | {r['sweep_accept_rate']:.2e} | {r['break_even_chain_steps']:.0f} | {r['nfold_ms_per_sweep_ms']:.2f} [{r['ratio_range'][0]:.2f} … {r['ratio_range'][1]:.2f}] | "
                     f"{q(r['energy_in'])} | {q(r['best_energy'])} | {q(r['sweep_best_energy'])} |")
    lines += ["", "µs per event is the launch time over the events of ALL chains (throughput, as the sweep's ns per chain-step is); the break-even is their quotient: the "
              "n-fold way is the faster one where fewer than one Metropolis step in that many is accepted."]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=4096)
    ap.add_argument("--Ns", type=int, nargs="+", default=[12, 15])
    ap.add_argument("--const-steps", type=int, default=100000)
    ap.add_argument("--ramp-steps", type=int, default=20000)
    ap.add_argument("--ramp-segs", type=int, default=20)
    ap.add_argument("--beta-end", type=float, default=3.0)
    ap.add_argument("--sweeps", type=int, default=200)
    ap.add_argument("--board-hops", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--resources-only", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile", default=None)
    args = ap.parse_args()

    import mcq_amd

    abi = mcq_amd.abi
    rep = {"resources": resources(mcq_amd), "lds": {str(n): abi.nfold3d_lds_bytes(n) for n in SHAPE_ENDS.values()}, "cases": [], "beta_end": args.beta_end}
    if not args.resources_only:
        import numpy as np
        import torch

        if mcq_amd._lib.device_count() < 1:
            raise RuntimeError("nfold3d_study needs a GPU (or --resources-only)")
        dev = torch.device("cuda", torch.cuda.current_device())
        n = args.chains
        seeds = abi.seeds_for(42, n)
        rep.update(chains=n, reps=args.reps, device=f"{torch.cuda.get_device_name(dev)} ({torch.cuda.get_device_properties(dev).gcnArchName})")
        sp = {"type": "linear_annealing", "beta_start": 1.0, "beta_end": 3.0}
        for N in args.Ns:
            rs = np.random.RandomState(42 + N)
            flat = np.stack([rs.choice(N ** 3, size=N * N, replace=False) for _ in range(n)])
            start = np.stack([flat // (N * N), (flat // N) % N, flat % N], axis=2).astype(np.uint8).reshape(n, -1)
            quenched = mcq_amd.quench.quench_queens(N, start, conflicts=False)["state"]
            ramp = abi.beta_values({"type": "linear_annealing", "beta_start": 1.0, "beta_end": args.beta_end}, args.ramp_steps)[:: args.ramp_steps // args.ramp_segs]
            rep["cases"].append(case(mcq_amd, torch, N, quenched, seeds, np.array([args.beta_end]), args.const_steps, "quenched random", args))
            rep["cases"].append(case(mcq_amd, torch, N, quenched, seeds, ramp, args.ramp_steps // args.ramp_segs, "quenched random", args))
            bath = mcq_amd.heatbath.anneal_heatbath(N, args.sweeps, "random", sp, seeds, mcmc_type="full_3d")["best_state"]
            bath = np.ascontiguousarray(bath, dtype=np.uint8).reshape(n, -1)
            rep["cases"].append(case(mcq_amd, torch, N, bath, seeds, np.array([args.beta_end]), args.const_steps,
                                     f"full_3d heat bath, {args.sweeps} sweeps (the cube's {PLATEAU.get(N, '?')})", args))
            sweeps, every = SWEEPS.get(N, (500, 5))
            res, _ = mcq_amd.heatbath.anneal_heatbath(N, sweeps, "random", sp, seeds, resample_every=every)
            hopped = mcq_amd.quench.hop_states(N, res["best_state"], seeds, args.board_hops, kick=2, local_search="pairs")
            plateau = np.ascontiguousarray(mcq_amd.quench.queens_of_boards(N, hopped["best_state"]), dtype=np.uint8).reshape(n, -1)
            rep["cases"].append(case(mcq_amd, torch, N, plateau, seeds, np.array([args.beta_end]), args.const_steps,
                                     f"board plateau: heat bath {sweeps} sweeps resampled every {every}, {args.board_hops} board hops, board best "
                                     f"{int(hopped['best_energy'].min())} (the cube's {PLATEAU.get(N, '?')})", args))
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
