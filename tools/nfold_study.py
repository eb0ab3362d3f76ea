#!/usr/bin/env python3
"""What the n-fold way costs per event, how many events a Metropolis step holds along a schedule, and how a whole run compares with
the Metropolis sweep on the same shape, on one MI355X (profiles/nfold.md).

    python tools/nfold_study.py [--chains 65536] [--Ns 12 15] [--n-steps 100000] [--seg-steps 1000] [--out FILE.json] [--profile profiles/nfold.md]

The setup of the other studies: board, random init, linear 1 -> 3, seeds 42 + r, no trace.  Per N, in one session:
  - anneal_nfold's launch alone (nfold_device on the reference's initial placements, every input on the device), timed by HIP events:
    the best and the worst of --reps launches after a warm-up, the events of the run (events_out) and from both the milliseconds per
    event of the launch, that is launch time / the sum of events over all chains;
  - the events per Metropolis step of every segment, from a second run cut at every segment boundary on the device (events_out less
    events_in, averaged over the chains, over seg_steps): the Metropolis acceptance rate along the schedule;
  - the Metropolis sweep of the same shape through run_experiment's path (experiments.run_chains, trace off), its kernel seconds, and
    from them the time per chain-step;
  - min / p10 / median of best_energy of both;
  - the break-even: the time per event over the sweep's time per chain-step, that is the number of Metropolis chain-steps an event
    costs.  A chain whose acceptance rate lies below the reciprocal of that figure spends less time per Metropolis step here than in
    the sweep.  Both are measured figures, not thresholds.
It also records the compiler's resource table of every instantiation of the kernel (VGPRs, LDS, scratch) from a compile of
csrc/mcq_nfold.hip with -Rpass-analysis=kernel-resource-usage; that part needs no GPU (--resources-only).
With --profile the section between the two `study` markers of that file is replaced by the tables."""
import argparse
import json
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BEGIN, END = "<!-- study:begin -->", "<!-- study:end -->"


def resources(mcq_amd):
    """{"NP": {vgprs, sgprs, lds, scratch, occupancy}} from the compiler's remarks."""
    b = mcq_amd.build
    cmd = [b.hipcc()] + [f for f in b.FLAGS if f != "-shared"] + ["-c", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-o", os.devnull, b.NFOLD_SOURCES[0]]
    err = subprocess.run(cmd, capture_output=True, text=True).stderr
    out, cur = {}, None
    for line in err.splitlines():
        m = re.search(r"Function Name: \S*mcq_nfold_kernelILi(\d+)E", line)
        if m:
            cur = out.setdefault(f"{int(m.group(1)):02d}", {})
        for key, pat in (("vgprs", r" VGPRs: (\d+)"), ("sgprs", r"TotalSGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)"),
                         ("vgpr_spills", r"VGPRs Spill: (\d+)"), ("sgpr_spills", r"SGPRs Spill: (\d+)")):
            m = re.search(pat, line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    return out


def quantiles(e):
    import numpy as np

    e = np.asarray(e)
    return {"min": int(e.min()), "p10": float(np.percentile(e, 10)), "median": float(np.median(e)), "mean": float(e.mean()), "max": int(e.max())}


def case(mcq_amd, torch, N, args):
    import numpy as np

    abi, nfold = mcq_amd.abi, mcq_amd.nfold
    sp = {"type": "linear_annealing", "beta_start": 1.0, "beta_end": 3.0}
    dev = torch.device("cuda", torch.cuda.current_device())
    st = torch.cuda.current_stream(dev)
    n, n_steps, seg = args.chains, args.n_steps, args.seg_steps
    n_segs = n_steps // seg
    seeds = abi.seeds_for(42, n)
    betas = np.ascontiguousarray(abi.beta_values(sp, n_steps)[::seg])
    first, _ = mcq_amd.experiments.start_chains(N, 0, "random", sp, seeds, mcmc_type="board", trace=False, states=True)
    start = torch.from_numpy(np.ascontiguousarray(first["final_state"], dtype=np.uint8).reshape(n, -1)).to(dev)
    dseeds = torch.from_numpy(seeds.view(np.int32)).to(dev)
    dtab = torch.from_numpy(nfold.weight_tables(betas).view(np.int32)).to(dev)
    ln2, ct = nfold.clock_tables(args.clock)
    clock = (ln2, torch.from_numpy(ct.view(np.int32)).to(dev))

    def launch():
        return nfold.nfold_device(N, start, dseeds, dtab, seg, clock=clock, stream=st)

    launch()  # warm-up
    st.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(args.reps):
        e0.record(st)
        res = launch()
        e1.record(st)
        st.synchronize()
        ms.append(e0.elapsed_time(e1))
    got = nfold.to_numpy(res)
    events = int(got["events_out"].sum())
    # the events of every segment: the same run cut at every boundary, need and event counter carried on the device
    state, need, ev, per_seg = start, None, None, []
    before = torch.zeros(n, dtype=torch.int64, device=dev)
    for s in range(n_segs):
        r = nfold.nfold_device(N, state, dseeds, dtab[s: s + 1], seg, first_seg=s, clock=clock, need_in=need, events_in=ev, stream=st)
        per_seg.append((r["events_out"] - before).double().mean())
        state, need, ev, before = r["state"], r["need_out"], r["events_out"], r["events_out"]
    st.synchronize()
    per_step = [float(x) / seg for x in per_seg]
    same = bool(np.array_equal(state.cpu().numpy(), got["state"]) and np.array_equal(ev.cpu().numpy(), got["events_out"]))
    # the Metropolis sweep of the same shape
    sweep_ms = []
    for _ in range(args.reps):
        met, secs = mcq_amd.experiments.run_chains(N, n_steps, "random", sp, seeds, mcmc_type="board", trace=False, states=False)
        sweep_ms.append(1e3 * float(secs))
    ms_per_event = min(ms) / max(events, 1)
    ms_per_chain_step = min(sweep_ms) / (n * n_steps)
    return {"N": N, "launch_ms": min(ms), "launch_worst_ms": max(ms), "events": events, "events_per_chain": events / n, "ms_per_event": ms_per_event,
            "events_per_step": per_step, "betas": [float(b) for b in betas], "cut_run_is_the_unbroken_run": same,
            "sweep_ms": min(sweep_ms), "sweep_worst_ms": max(sweep_ms), "ms_per_chain_step": ms_per_chain_step,
            "chain_steps_per_event": ms_per_event / ms_per_chain_step, "break_even_acceptance": ms_per_chain_step / ms_per_event, "acceptance_whole_run": events / (n * n_steps),
            "nfold_best_energy": quantiles(got["best_energy"]), "sweep_best_energy": quantiles(met["best_energy"]),
            "uphill_share": float(got["n_uphill"].sum()) / max(events, 1), "flat_share": float(got["n_flat"].sum()) / max(events, 1)}


def markdown(rep):
    q = lambda d: f"{d['min']} / {d['p10']:g} / {d['median']:g}"  # noqa: E731
    lines = ["Compiler's resource table of `csrc/mcq_nfold.hip` (`-Rpass-analysis=kernel-resource-usage`, gfx950):", "",
             "| instantiation NP | VGPRs | SGPRs | VGPRs spilled | SGPRs spilled (to VGPR lanes) | LDS bytes per chain | scratch bytes per lane | waves per SIMD |", "|---|---|---|---|---|---|---|---|"]
    for NP, r in sorted(rep["resources"].items()):
        lines.append(f"| {NP.lstrip('0')} | {r.get('vgprs')} | {r.get('sgprs')} | {r.get('vgpr_spills')} | {r.get('sgpr_spills')} | {r.get('lds')} | {r.get('scratch')} | {r.get('occupancy')} |")
    lines += ["", "No instantiation uses scratch." if not any(r.get("scratch") for r in rep["resources"].values()) else "Some instantiations use scratch: see the table."]
    if not rep.get("cases"):
        return "\n".join(lines + ["", "Not measured: no GPU session was had for the figures below the resource table."])
    lines += ["", f"Measured by `tools/nfold_study.py` in one session on one {rep['device']}: {rep['chains']} board chains, random init, linear 1 → 3 over {rep['n_steps']} "
              f"Metropolis steps in segments of {rep['seg_steps']}, seeds 42 + r, clock `{rep['clock']}`. The n-fold launch is timed by HIP events, the best of {rep['reps']} launches "
              "after a warm-up with the worst in brackets; the Metropolis sweep is the sweep kernel's own time over the same number of runs.", "",
              "| N | n-fold launch, ms | events per chain | ms per event (launch / all events) | Metropolis sweep, ms | ms per chain-step | chain-steps an event costs (ms per event / ms per chain-step) | break-even acceptance rate (its reciprocal) | acceptance rate of the whole run | "
              "share of events uphill / flat | n-fold `best_energy` min / p10 / median | sweep `best_energy` min / p10 / median |", "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    ok = True
    for c in rep["cases"]:
        ok = ok and c["cut_run_is_the_unbroken_run"]
        lines.append(f"| {c['N']} | {c['launch_ms']:.1f} ({c['launch_worst_ms']:.1f}) | {c['events_per_chain']:.0f} | {c['ms_per_event']:.3e} | {c['sweep_ms']:.1f} ({c['sweep_worst_ms']:.1f}) | "
                     f"{c['ms_per_chain_step']:.3e} | {c['chain_steps_per_event']:.2f} | {c['break_even_acceptance']:.4f} | {c['acceptance_whole_run']:.4f} | {c['uphill_share']:.3f} / {c['flat_share']:.3f} | "
                     f"{q(c['nfold_best_energy'])} | {q(c['sweep_best_energy'])} |")
    lines += ["", "### Events per Metropolis step along the schedule", "",
              "The mean over the chains of the events of a segment over its Metropolis steps: the acceptance rate of the Metropolis chain at that beta. About ten segments along the schedule:", "",
              "| N | " + " | ".join(f"β = {b:.2f}" for b in rep["cases"][0]["betas"][::max(1, len(rep['cases'][0]['betas']) // 10)]) + " |",
              "|---|" + "---|" * len(rep["cases"][0]["betas"][::max(1, len(rep['cases'][0]['betas']) // 10)])]
    for c in rep["cases"]:
        lines.append(f"| {c['N']} | " + " | ".join(f"{x:.4f}" for x in c["events_per_step"][::max(1, len(c['events_per_step']) // 10)]) + " |")
    lines += ["", "In every case the run cut at every segment boundary on the device ended on the placements and the event counters of the one launch."
              if ok else "NOT every cut run equalled the unbroken one: see the JSON."]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=65536)
    ap.add_argument("--Ns", type=int, nargs="+", default=[12, 15])
    ap.add_argument("--n-steps", type=int, default=100000)
    ap.add_argument("--seg-steps", type=int, default=1000)
    ap.add_argument("--clock", default="exp")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--resources-only", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile", default=None)
    args = ap.parse_args()
    if args.n_steps % args.seg_steps:
        ap.error("--n-steps must be a multiple of --seg-steps")

    import mcq_amd

    rep = {"resources": resources(mcq_amd), "cases": []}
    if not args.resources_only:
        import torch

        if mcq_amd._lib.device_count() < 1:
            raise RuntimeError("nfold_study needs a GPU (or --resources-only)")
        dev = torch.device("cuda", torch.cuda.current_device())
        rep.update(chains=args.chains, n_steps=args.n_steps, seg_steps=args.seg_steps, clock=args.clock, reps=args.reps, device=torch.cuda.get_device_name(dev))
        for N in args.Ns:
            rep["cases"].append(case(mcq_amd, torch, N, args))
            print(json.dumps(rep["cases"][-1]), flush=True)
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
