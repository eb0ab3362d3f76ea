#!/usr/bin/env python3
"""Parallel tempering of the full_3d heat-bath queen sweep next to the plain queen sweep, on one MI355X: writes profiles/tempering3d.md.

    python tools/tempering3d_study.py [--chains 4096] [--Ns 12 15] [--sweeps 50 30] [--probe 5] [--reps 3] [--lo 0.6] [--hi 1.4]
                                      [--out profiles/tempering3d.md] [--json FILE.json] [--resources-only]

full_3d, Q = N^2, random init (the reference's own initial placements of the seeds 42 + r), linear beta 1 -> 3 per sweep, no trace, all in
one process:
  cost    ms per sweep of mcq_temper3d_device at R = 16 and R = 4, K = 1 (HIP events around one call of --probe sweeps, best of --reps
          after a warm-up), next to mcq_heatbath3d_device on the same placements, chain count and sweep count.  The chains of a ladder
          are narrower than the plain kernel's wherever R W would pass 1 024 lanes, so this is the cost of the layout, not of the
          exchange alone.
  effect  min / p10 / median best_energy over all slots and over the slots that END on the coldest rung at --sweeps sweeps, ladder =
          linspace(--lo, --hi, R), K = 1, next to anneal_heatbath(mcmc_type="full_3d") at equal sweeps; per-pair acceptance rates.
--resources-only (no GPU): the register / LDS table of the seven instantiations from hipcc -Rpass-analysis=kernel-resource-usage, and the
statement that no timing or energy figure is on record.  Either way the tool FAILS if an instantiation reports scratch."""
import argparse
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (W, BITS, STEPS) -> (the N it serves at Q = N^2 and table_len = 512, the R it serves)
SERVES = {(64, 8, 32): ("2 … 12", "2, 4, 8, 16"), (256, 8, 64): ("13 … 19", "2, 4"), (128, 8, 64): ("13 … 19", "8"), (64, 8, 64): ("13 … 18", "16"),
          (512, 16, 64): ("20 … 32", "2"), (256, 16, 64): ("20 … 25", "4"), (128, 16, 64): ("20", "8")}


def resources():
    """[(W, BITS, STEPS, vgprs, sgprs, scratch, occupancy, static LDS)] of mcq_temper3d_kernel<W, BITS, STEPS>, from the compiler's remarks."""
    import mcq_amd

    b = mcq_amd.build
    cmd = [b.hipcc()] + [f for f in b.FLAGS if f != "-shared"] + ["--cuda-device-only", "-c", "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"] + b.TEMPER3D_SOURCES
    err = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    rows = []
    for block in err.split("Function Name: ")[1:]:
        m = re.match(r"\S*mcq_temper3d_kernelILi(\d+)ELi(\d+)ELi(\d+)E", block)
        if not m:
            continue
        get = lambda key: int(re.search(key + r":\s*(\d+)", block).group(1))  # noqa: E731
        rows.append(tuple(int(x) for x in m.groups()) + (get("VGPRs"), get("TotalSGPRs"), get(r"ScratchSize \[bytes/lane\]"), get(r"Occupancy \[waves/SIMD\]"),
                                                         get(r"LDS Size \[bytes/block\]")))
    rows.sort(key=lambda r: (r[1], r[2], -r[0]))
    if sorted(r[:3] for r in rows) != sorted(SERVES):
        raise SystemExit(f"tempering3d_study: expected the seven instantiations {sorted(SERVES)}, the compiler reports {sorted(r[:3] for r in rows)}")
    spilled = [r[:3] for r in rows if r[5] != 0]
    if spilled:
        raise SystemExit(f"tempering3d_study: SCRATCH in {spilled}: a spill in the queen update is a regression, not a figure to record")
    return rows


def resource_table():
    import mcq_amd

    abi = mcq_amd.abi
    lines = ["| instantiation `<W, BITS, STEPS>` | serves N (Q = N², D = 512) | with R | VGPRs | SGPRs | scratch | wavefronts per SIMD by registers | static LDS |", "|---|---|---|---|---|---|---|---|"]
    for W, bits, steps, v, s, scratch, occ, lds in resources():
        n, r = SERVES[(W, bits, steps)]
        lines.append(f"| `<{W}, {bits}, {steps}>` | {n} | {r} | {v} | {s} | {scratch} | {occ} | {lds} B |")
    limit = abi.MAX_TEMPER_LDS - abi.TEMPER3D_STATIC_LDS
    lines += ["", "Dynamic LDS of a ladder at Q = N², D = 512 (`abi.temper3d_lds_bytes`; refused above " + f"{limit:,} B):".replace(",", " "), "",
              "| N | R = 2 | R = 4 | R = 8 | R = 16 |", "|---|---|---|---|---|"]
    for N in (4, 8, 12, 13, 16, 18, 19, 20, 21, 24, 25, 26, 32):
        cells = [f"{abi.temper3d_lds_bytes(N, R):,}".replace(",", " ") + (" (refused)" if abi.temper3d_lds_bytes(N, R) > limit else "") for R in (2, 4, 8, 16)]
        lines.append(f"| {N} | " + " | ".join(cells) + " |")
    return "\n".join(lines)


def quantiles(e):
    import numpy as np

    return {"min": int(e.min()), "p10": float(np.percentile(e, 10)), "median": float(np.median(e))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=4096)
    ap.add_argument("--Ns", type=int, nargs="+", default=[12, 15])
    ap.add_argument("--sweeps", type=int, nargs="+", default=[50, 30])
    ap.add_argument("--probe", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--lo", type=float, default=0.6)
    ap.add_argument("--hi", type=float, default=1.4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tempering3d.md"))
    ap.add_argument("--json", default=None)
    ap.add_argument("--resources-only", action="store_true")
    args = ap.parse_args()

    head = ["# Parallel tempering of the full_3d heat-bath queen sweep (`mcq_temper3d_device`, DESIGN.md §4.12)", ""]
    res_part = ["## Resources", "",
                "`hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage`, the seven instantiations `mcq_temper3d_kernel<W, BITS, STEPS>` (lanes per chain,",
                "bits per field entry, steps per direction of an update). A workgroup is one ladder of R·W ≤ 1 024 lanes, so the kernel is compiled for 1 024 lanes, which caps",
                "it at 128 VGPRs. The static LDS is the scratch of the workgroup-wide OR behind \"some slot repeats\"; everything else is dynamic.", "",
                resource_table(), "", "No scratch in any of them (the tool fails otherwise).", ""]
    if args.resources_only:
        text = head + ["**No timing or energy figure is on record**: `python tools/tempering3d_study.py` has not been run on a GPU in this tree. What follows is what the compiler",
                       "reports, without a GPU (`python tools/tempering3d_study.py --resources-only` wrote this file).", ""] + res_part
        with open(args.out, "w") as f:
            f.write("\n".join(text))
        print(args.out)
        return

    import numpy as np
    import torch

    import mcq_amd

    abi, hb, tp = mcq_amd.abi, mcq_amd.heatbath, mcq_amd.tempering
    if mcq_amd._lib.device_count() < 1:
        raise RuntimeError("tempering3d_study needs a GPU (--resources-only runs without one)")
    sp = {"type": "linear_annealing", "beta_start": 1.0, "beta_end": 3.0}
    st = torch.cuda.current_stream()
    dev = torch.device("cuda", torch.cuda.current_device())
    n = args.chains
    seeds = abi.seeds_for(42, n)
    dseeds = torch.from_numpy(seeds.view(np.int32).copy()).to(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn):
        e0.record(st)
        out = fn()
        e1.record(st)
        st.synchronize()
        return out, e0.elapsed_time(e1)

    report = {"chains": n, "device": torch.cuda.get_device_name(dev), "ladder": [args.lo, args.hi], "cases": []}
    cost = ["## Cost of a sweep", "", f"{n:,}".replace(",", " ") + f" chains, Q = N², K = 1, one call of {args.probe} sweeps 1 → 3, best of {args.reps} by HIP events after a warm-up; ms per sweep.", "",
            "| N | `heatbath_queens_device` | tempered, R = 4 | tempered, R = 16 |", "|---|---|---|---|"]
    effect = ["## Effect", "", "`best_energy` (min / p10 / median) of " + f"{n:,}".replace(",", " ") + f" slots, ladder linspace({args.lo}, {args.hi}, R), K = 1; \"coldest\" = the slots that end on rung R − 1;",
              "the plain sweep is `anneal_heatbath(mcmc_type=\"full_3d\")` on the same seeds at the same number of sweeps.", "",
              "| N | sweeps | plain sweep | R = 4, all slots | R = 4, coldest | R = 16, all slots | R = 16, coldest | kernel ms (R = 4 / R = 16) |", "|---|---|---|---|---|---|---|---|"]
    rates = ["## Acceptance per pair of rungs", ""]
    fmt = lambda q: f"{q['min']} / {q['p10']:g} / {q['median']:g}"  # noqa: E731
    for N, n_sweeps in zip(args.Ns, args.sweeps):
        first, _ = mcq_amd.experiments.start_chains(N, 0, "random", sp, seeds, mcmc_type="full_3d", trace=False, states=True, Q=N * N)
        start = torch.from_numpy(np.ascontiguousarray(first["final_state"], dtype=np.uint8).reshape(n, -1)).to(dev)
        case = {"N": N, "ms_per_sweep": {}}

        def plain(k):
            tab = hb.device_table(abi.beta_values(sp, k), dev)
            st.synchronize()
            return timed(lambda: hb.heatbath_queens_device(N, start, dseeds, tab, stream=st))

        def tempered(k, R):
            tabs = tp.device_tables(abi.beta_values(sp, k), np.linspace(args.lo, args.hi, R), 1, 0, dev)
            st.synchronize()
            return timed(lambda: tp.temper_queens_device(N, start, dseeds, tables=tabs, stream=st))

        plain(2), tempered(2, 4), tempered(2, 16)  # warm-up: loads the code objects
        case["ms_per_sweep"]["plain"] = min(plain(args.probe)[1] for _ in range(args.reps)) / args.probe
        for R in (4, 16):
            case["ms_per_sweep"][f"R{R}"] = min(tempered(args.probe, R)[1] for _ in range(args.reps)) / args.probe
        m = case["ms_per_sweep"]
        cost.append(f"| {N} | {m['plain']:.3f} | {m['R4']:.3f} ({m['R4'] / m['plain'] - 1:+.1%}) | {m['R16']:.3f} ({m['R16'] / m['plain'] - 1:+.1%}) |")
        base = hb.anneal_heatbath(N, n_sweeps, "random", sp, seeds, mcmc_type="full_3d")
        run = {"sweeps": n_sweeps, "plain": quantiles(base["best_energy"])}
        for R in (4, 16):
            res, ms = tempered(n_sweeps, R)
            got = tp.to_numpy(res)
            cold = got["rung_out"] == R - 1
            stats = tp.ladder_statistics(got, ((n_sweeps + 1) // 2, n_sweeps // 2))
            run[f"R{R}"] = {"all": quantiles(got["best_energy"]), "coldest": quantiles(got["best_energy"][cold]), "ms": ms,
                            "pair_rate": [float(x) for x in stats["pair_rate"]], "exchanges_per_slot": stats["exchanges_per_slot"]}
            rates.append(f"* N = {N}, {n_sweeps} sweeps, R = {R}: " + " ".join(f"{x:.2f}" for x in stats["pair_rate"]) + f" ({stats['exchanges_per_slot']:.1f} swaps per slot)")
        effect.append(f"| {N} | {n_sweeps} | {fmt(run['plain'])} | {fmt(run['R4']['all'])} | {fmt(run['R4']['coldest'])} | {fmt(run['R16']['all'])} | {fmt(run['R16']['coldest'])} | "
                      f"{run['R4']['ms']:.1f} / {run['R16']['ms']:.1f} |")
        case["run"] = run
        report["cases"].append(case)
        print(json.dumps(case), flush=True)
    text = head + [f"One session on one {report['device']}, one process: `python tools/tempering3d_study.py` wrote this file.", ""] + cost + [""] + effect + [""] + rates + [""] + res_part
    with open(args.out, "w") as f:
        f.write("\n".join(text))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(report, f, indent=1)
    print(args.out)


if __name__ == "__main__":
    main()
