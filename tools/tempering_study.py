#!/usr/bin/env python3
"""Parallel tempering of the board heat-bath sweep next to the plain sweep, on one MI355X: writes profiles/tempering.md.

    python tools/tempering_study.py [--chains 65536] [--Ns 12 15] [--short 89 62] [--long 700 445] [--probe 20] [--reps 3]
                                    [--lo 0.6] [--hi 1.4] [--out profiles/tempering.md] [--json FILE.json] [--resources-only]
    python tools/tempering_study.py --ab 8 12 15 16 [--chains 65536] [--out profiles/tempering_counters.md]      (and a JSON next to it)

Board, random init (the reference's own initial placements of the seeds 42 + r), linear beta 1 -> 3 per sweep, no trace, all in one process:
  cost    ms per sweep of mcq_temper_device at R = 16 and R = 4, K = 1 (HIP events around one call of --probe sweeps, best of --reps
          after a warm-up), next to mcq_heatbath_device on the same placements, chain count and sweep count.  What the exchange costs
          is that difference; the R staged table rows, the two barriers per event and the occupancy of the larger workgroups (the
          resource table) account for it.
  effect  min / p10 / median best_energy over all slots and over the slots that END on the coldest rung, at the sweep counts of
          profiles/heatbath.md (--short: its equal-time counts, --long: its fixed counts), ladder = linspace(--lo, --hi, R), K = 1,
          next to the plain sweep at the same counts; per-pair acceptance rates from pair_accepted.
--ab is a timing leg of its own, the two forms of the tempered sweep (tempering.FORMS) in one process: per N and for R = 4 and R = 16,
--chains random boards, the same seeds and tables for both forms, one call of --probe sweeps 1 -> 3 at K = 1, the best of --reps calls by
HIP events after a warm-up, the forms alternated (lines, counters, lines, counters); the sums of energy_out, n_changed and pair_accepted
of the two forms must be equal.  The spread between the two rounds of one form is the noise of the figure: a difference inside it is
"level".  Next to the times: the resource table of the counter kernel's twelve instantiations and the ladders a CU holds by LDS and by
registers.
--resources-only (no GPU): the register / LDS table of the six instantiations from hipcc -Rpass-analysis=kernel-resource-usage, and the
statement that no timing or energy figure is on record."""
import argparse
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HAND = "## Recorded by hand"  # --ab keeps what profiles/tempering_counters.md holds from this heading on
SERVES = {8: "2 … 8", 12: "9 … 12", 16: "13 … 16", 24: "17 … 24", 32: "25 … 32", 64: "33 … 64"}


def resources(kernel="mcq_temper_kernel"):
    """[(GW, NP, vgprs, sgprs, scratch, occupancy)] of mcq_temper_kernel<GW, NP>, from the compiler's remarks; with
    kernel="mcq_temper_counters_kernel" the rows are (NP, R, ...) of mcq_temper_counters_kernel<NP, R>, sorted by (NP, R)."""
    import mcq_amd

    b = mcq_amd.build
    cmd = [b.hipcc()] + [f for f in b.FLAGS if f != "-shared"] + ["--cuda-device-only", "-c", "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"] + b.TEMPER_SOURCES
    err = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    rows = []
    for block in err.split("Function Name: ")[1:]:
        m = re.match(r"\S*\d" + kernel + r"ILi(\d+)ELi(\d+)E", block)
        if not m:
            continue
        get = lambda key: int(re.search(key + r":\s*(\d+)", block).group(1))  # noqa: E731
        rows.append((int(m.group(1)), int(m.group(2)), get("VGPRs"), get("TotalSGPRs"), get(r"ScratchSize \[bytes/lane\]"), get(r"Occupancy \[waves/SIMD\]")))
    return sorted(rows, key=lambda r: r[1]) if kernel == "mcq_temper_kernel" else sorted(rows)


def resource_table(D=20):
    lines = ["| instantiation | serves N | VGPRs | SGPRs | scratch | wavefronts per SIMD by registers | LDS of a ladder at R = 2 / 4 / 8 / 16 (D = %d) |" % D,
             "|---|---|---|---|---|---|---|"]
    for GW, NP, v, s, scratch, occ in resources():
        lds = " / ".join(f"{(R * 6 * NP * NP + 4 * R * D + 12 * R + 15) // 16 * 16:,}".replace(",", " ") + (" (refused)" if R * 6 * NP * NP > 160 * 1024 else "")
                         for R in (2, 4, 8, 16))
        lines.append(f"| `<{GW}, {NP}>` | {SERVES[NP]} | {v} | {s} | {scratch} | {occ} | {lds} B |")
    return "\n".join(lines)


def counters_resource_table(D):
    """The twelve instantiations of mcq_temper_counters_kernel<NP, R>: registers, the LDS of a workgroup at table_len = D and at 512, and
    the ladders a CU holds by LDS (160 KiB) and by registers (512 VGPRs per SIMD lane in blocks of 8, 4 SIMDs)."""
    import mcq_amd

    lds = mcq_amd.abi.temper_counters_lds_bytes
    sp = lambda x: f"{x:,}".replace(",", " ")  # noqa: E731
    lines = [f"| instantiation | serves N | lanes of a workgroup (ladders) | VGPRs | SGPRs | scratch | LDS of a workgroup, D = {D} / 512 | ladders per CU by LDS, D = {D} / 512 | ladders per CU by registers |",
             "|---|---|---|---|---|---|---|---|---|"]
    rows = resources("mcq_temper_counters_kernel")
    for NP, R, v, s, scratch, occ in rows:
        threads, lpb = max(64, 16 * R), 2 if R == 2 else 1
        waves = (512 // ((v + 7) // 8 * 8)) * 4  # wavefronts a CU holds by VGPRs
        by_regs = min(waves // (threads // 64), 32) * lpb
        a, b = lds(NP, R, D), lds(NP, R, 512)
        lines.append(f"| `<{NP}, {R}>` | {SERVES[NP]} | {threads} ({lpb}) | {v} | {s} | {scratch} | {sp(a)} / {sp(b)} B | {160 * 1024 // a * lpb} / {160 * 1024 // b * lpb} | {by_regs} |")
    return "\n".join(lines), rows


def ab(args):
    """The two forms of the tempered sweep next to each other: writes args.out (profiles/tempering_counters.md) and a JSON next to it."""
    import numpy as np
    import torch

    import mcq_amd
    from tests import quench_util as qu

    abi, tp = mcq_amd.abi, mcq_amd.tempering
    sp = {"type": "linear_annealing", "beta_start": 1.0, "beta_end": 3.0}
    n = args.chains
    betas = abi.beta_values(sp, args.probe)
    if args.resources_only:
        D = max(abi.temper_tables(betas, np.linspace(args.lo, args.hi, R), 1, 0)[0].shape[2] for R in (4, 16))
        return write_ab(args, {"chains": n, "device": None, "sweeps": args.probe, "reps": args.reps, "ladder": [args.lo, args.hi], "ab": []}, D)
    if mcq_amd._lib.device_count() < 1:
        raise RuntimeError("tempering_study --ab needs a GPU (with --resources-only it writes the resource table without one)")
    st = torch.cuda.current_stream()
    dev = torch.device("cuda", torch.cuda.current_device())
    dseeds = torch.from_numpy(abi.seeds_for(42, n).view(np.int32).copy()).to(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn):
        e0.record(st)
        out = fn()
        e1.record(st)
        st.synchronize()
        return out, e0.elapsed_time(e1)

    report = {"chains": n, "device": torch.cuda.get_device_name(dev), "sweeps": args.probe, "reps": args.reps, "ladder": [args.lo, args.hi], "ab": []}
    for N in args.ab:
        start = torch.from_numpy(qu.random_boards(N, n, N)).to(dev)
        for R in (4, 16):
            tabs = tp.device_tables(betas, np.linspace(args.lo, args.hi, R), 1, 0, dev)
            case = {"N": N, "R": R, "table_len": int(tabs[0].shape[2]), "lines_ms_per_sweep": [], "counters_ms_per_sweep": []}
            sums = {}
            for rnd in range(2):
                for form in tp.FORMS:
                    tp.temper_device(N, start, dseeds, tables=(tabs[0][:2], tabs[1][:2]), stream=st, form=form)  # warm-up
                    st.synchronize()
                    runs = [timed(lambda: tp.temper_device(N, start, dseeds, tables=tabs, stream=st, form=form)) for _ in range(args.reps)]
                    case[form + "_ms_per_sweep"].append(min(ms for _, ms in runs) / args.probe)
                    res = runs[-1][0]
                    sums.setdefault(form, []).append(tuple(int(res[k].sum().item()) for k in ("energy_out", "n_changed", "pair_accepted")))
            assert len(set(sums["lines"] + sums["counters"])) == 1, f"N={N} R={R}: the two forms disagree: {sums}"
            case["energy_out_sum"], case["n_changed_sum"], case["pair_accepted_sum"] = sums["lines"][0]
            lo, co = case["lines_ms_per_sweep"], case["counters_ms_per_sweep"]
            case["change"] = min(co) / min(lo) - 1.0
            case["spread"] = max(max(lo) / min(lo), max(co) / min(co)) - 1.0
            case["verdict"] = "level" if abs(case["change"]) <= case["spread"] else "counters" if case["change"] < 0 else "lines"
            report["ab"].append(case)
            print(json.dumps(case), flush=True)
    write_ab(args, report, max(c["table_len"] for c in report["ab"]))


def write_ab(args, report, D):
    """profiles/tempering_counters.md and the JSON next to it from a report; no case in it means that nothing was measured."""
    n = report["chains"]
    num = lambda x: f"{x:,}".replace(",", " ")  # noqa: E731
    table, rows = counters_resource_table(D)
    report["resources"] = [dict(zip(("NP", "R", "vgprs", "sgprs", "scratch", "occupancy"), r)) for r in rows]
    two = lambda v: " / ".join(f"{x:.3f}" for x in v)  # noqa: E731
    says = {"level": "level", "counters": "`\"counters\"` faster", "lines": "`\"lines\"` faster"}
    head = ["# The counter form of the tempered board sweep (`mcq_temper_counters_device`, DESIGN.md §4.11)", ""]
    cmd = "`python tools/tempering_study.py --ab " + " ".join(str(N) for N in args.ab)
    if not report["ab"]:
        text = head + ["## Measured on the GPU", "",
                       f"**Not yet: no timing of this kernel is on record.** {cmd}` has not run on a GPU in this tree; it writes the milliseconds per sweep of both forms here",
                       f"({num(n)} random boards, R = 4 and R = 16, K = 1, {args.probe} sweeps 1 → 3, best of {args.reps} by HIP events, the forms alternated twice, equal sums asserted). Whether",
                       f"`\"counters\"` is faster, and for which N and R, is not known. What follows is what the compiler reports, without a GPU ({cmd} --resources-only` wrote it).", ""]
    else:
        text = head + [
            f"One session on one {report['device']}, one process: {cmd}` wrote this part of the file.", "",
            "## Measured: ms per sweep, lines against counters", "",
            f"{num(n)} random boards ({num(n // 4)} ladders at R = 4, {num(n // 16)} at R = 16), the same boards, seeds and tables for both forms, ladder linspace({args.lo}, {args.hi}, R), K = 1, one call of",
            f"{args.probe} sweeps 1 → 3, best of {args.reps} by HIP events after a warm-up, the forms alternated (lines, counters, lines, counters): two figures per form. Equal sums of `energy_out`,",
            "`n_changed` and `pair_accepted` were asserted between the forms. The spread between the two rounds of one form is the noise; a difference inside it is \"level\".", "",
            "| N | R | `\"lines\"`, rounds 1 / 2 | `\"counters\"`, rounds 1 / 2 | best counters against best lines | spread of the rounds | reading |", "|---|---|---|---|---|---|---|"]
    for c in report["ab"]:
        text.append(f"| {c['N']} | {c['R']} | {two(c['lines_ms_per_sweep'])} | {two(c['counters_ms_per_sweep'])} | {c['change']:+.1%} | {c['spread']:.1%} | {says[c['verdict']]} |")
    text += ["", "## Resources", "",
             "`hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -Rpass-analysis=kernel-resource-usage` on `csrc/mcq_temper.hip`, the twelve instantiations `mcq_temper_counters_kernel<NP, R>`",
             "(padding class, replicas), each compiled with the `__launch_bounds__` of its real workgroup. The LDS is dynamic: per ladder R regions of 1 856 / 4 288 / 7 616 bytes, 4·R·D bytes of",
             f"staged rows (D = `table_len`: {D} with the tool's tables, at most 512) and 12·R bytes for the event; two ladders per workgroup at R = 2.", "", table, ""]
    if os.path.exists(args.out):  # what was written by hand below the marker stays
        old = open(args.out).read()
        if HAND in old:
            text.append(old[old.index(HAND):])
    with open(args.out, "w") as f:
        f.write("\n".join(text))
    with open(os.path.splitext(args.out)[0] + ".json", "w") as f:
        json.dump(report, f, indent=1)
    print(args.out)


def quantiles(e):
    import numpy as np

    return {"min": int(e.min()), "p10": float(np.percentile(e, 10)), "median": float(np.median(e))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=65536)
    ap.add_argument("--Ns", type=int, nargs="+", default=[12, 15])
    ap.add_argument("--short", type=int, nargs="+", default=[89, 62])
    ap.add_argument("--long", type=int, nargs="+", default=[700, 445])
    ap.add_argument("--probe", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--lo", type=float, default=0.6)
    ap.add_argument("--hi", type=float, default=1.4)
    ap.add_argument("--out", default=None)
    ap.add_argument("--json", default=None)
    ap.add_argument("--resources-only", action="store_true")
    ap.add_argument("--ab", type=int, nargs="+", default=None, metavar="N")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "tempering.md" if args.ab is None else "tempering_counters.md")
    if args.ab is not None:
        return ab(args)

    head = ["# Parallel tempering of the board heat-bath sweep (`mcq_temper_device`, DESIGN.md §4.11)", ""]
    res_part = ["## Resources", "",
                "`hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage`, the six instantiations `mcq_temper_kernel<GW, NP>` (lanes per chain, line padding in",
                "bytes). A workgroup is one ladder of R·GW lanes (two ladders for R = 2 at N ≤ 16), so the kernel is compiled for up to 1 024 lanes, which caps it at 128 VGPRs;",
                "the LDS is dynamic: 6·NP²·R bytes of placements, 4·R·D bytes of staged table rows (D = `table_len`, at most 512) and 12·R bytes for the event.", "",
                resource_table(), "",
                "No scratch in any of them. The plain kernel's instantiations for N > 24 use 168 and 173 VGPRs (`profiles/heatbath.md`); here they are held to 110 and 115.", ""]
    if args.resources_only:
        text = head + ["**No timing or energy figure is on record**: `python tools/tempering_study.py` has not been run on a GPU in this tree. What follows is what the compiler",
                       "reports, without a GPU (`python tools/tempering_study.py --resources-only` wrote this file).", ""] + res_part
        with open(args.out, "w") as f:
            f.write("\n".join(text))
        print(args.out)
        return

    import numpy as np
    import torch

    import mcq_amd

    abi, hb, tp = mcq_amd.abi, mcq_amd.heatbath, mcq_amd.tempering
    if mcq_amd._lib.device_count() < 1:
        raise RuntimeError("tempering_study needs a GPU (--resources-only runs without one)")
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
    cost = ["## Cost of a sweep", "", f"{n:,} chains, K = 1, one call of {args.probe} sweeps 1 → 3, best of {args.reps} by HIP events after a warm-up; ms per sweep.".replace(",", " "), "",
            "| N | `heatbath_device` | tempered, R = 4 | tempered, R = 16 |", "|---|---|---|---|"]
    effect = ["## Effect", "", f"`best_energy` (min / p10 / median) of {n:,} slots, ladder linspace({args.lo}, {args.hi}, R), K = 1; \"coldest\" = the slots that end on rung R − 1.".replace(",", " "),
              "The plain and resampled figures of `profiles/heatbath.md` at the same sweep counts are its rows (b) and (c).", "",
              "| N | sweeps | plain sweep (this session) | R = 4, all slots | R = 4, coldest | R = 16, all slots | R = 16, coldest | kernel ms (plain / R = 4 / R = 16) |",
              "|---|---|---|---|---|---|---|---|"]
    rates = ["## Acceptance per pair of rungs", ""]
    fmt = lambda q: f"{q['min']} / {q['p10']:g} / {q['median']:g}"  # noqa: E731
    for N, short, long_ in zip(args.Ns, args.short, args.long):
        first, _ = mcq_amd.experiments.start_chains(N, 0, "random", sp, seeds, mcmc_type="board", trace=False, states=True)
        start = torch.from_numpy(np.ascontiguousarray(first["final_state"])).to(dev)
        case = {"N": N, "ms_per_sweep": {}, "runs": []}

        def plain(n_sweeps):
            tab = hb.device_table(abi.beta_values(sp, n_sweeps), dev)
            st.synchronize()
            return timed(lambda: hb.heatbath_device(N, start, dseeds, tab, stream=st))

        def tempered(n_sweeps, R):
            tabs = tp.device_tables(abi.beta_values(sp, n_sweeps), np.linspace(args.lo, args.hi, R), 1, 0, dev)
            st.synchronize()
            return timed(lambda: tp.temper_device(N, start, dseeds, tables=tabs, stream=st))

        plain(2), tempered(2, 4), tempered(2, 16)  # warm-up: loads the code objects
        case["ms_per_sweep"]["plain"] = min(plain(args.probe)[1] for _ in range(args.reps)) / args.probe
        for R in (4, 16):
            case["ms_per_sweep"][f"R{R}"] = min(tempered(args.probe, R)[1] for _ in range(args.reps)) / args.probe
        m = case["ms_per_sweep"]
        cost.append(f"| {N} | {m['plain']:.3f} | {m['R4']:.3f} ({m['R4'] / m['plain'] - 1:+.1%}) | {m['R16']:.3f} ({m['R16'] / m['plain'] - 1:+.1%}) |")
        for n_sweeps in (short, long_):
            res, ms = plain(n_sweeps)
            run = {"sweeps": n_sweeps, "plain": quantiles(res["best_energy"].cpu().numpy()), "plain_ms": ms}
            for R in (4, 16):
                res, ms = tempered(n_sweeps, R)
                got = tp.to_numpy(res)
                cold = got["rung_out"] == R - 1
                events = n_sweeps
                stats = tp.ladder_statistics(got, ((events + 1) // 2, events // 2))
                run[f"R{R}"] = {"all": quantiles(got["best_energy"]), "coldest": quantiles(got["best_energy"][cold]), "ms": ms,
                                "pair_rate": [float(x) for x in stats["pair_rate"]], "exchanges_per_slot": stats["exchanges_per_slot"]}
                rates.append(f"* N = {N}, {n_sweeps} sweeps, R = {R}: " + " ".join(f"{x:.2f}" for x in stats["pair_rate"]) + f" ({stats['exchanges_per_slot']:.1f} swaps per slot)")
            effect.append(f"| {N} | {n_sweeps} | {fmt(run['plain'])} | {fmt(run['R4']['all'])} | {fmt(run['R4']['coldest'])} | {fmt(run['R16']['all'])} | {fmt(run['R16']['coldest'])} | "
                          f"{run['plain_ms']:.1f} / {run['R4']['ms']:.1f} / {run['R16']['ms']:.1f} |")
            case["runs"].append(run)
        report["cases"].append(case)
        print(json.dumps(case), flush=True)
    text = head + [f"One session on one {report['device']}, one process: `python tools/tempering_study.py` wrote this file.", ""] + cost + [""] + effect + [""] + rates + [""] + res_part
    with open(args.out, "w") as f:
        f.write("\n".join(text))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(report, f, indent=1)
    print(args.out)


if __name__ == "__main__":
    main()
