"""Derives the case table of tests/variant_cases.py: `python -m tools.derive_variant_cases` prints it, `--write` puts it between the
two markers of that file.  Needs the built library and the oracle, no GPU (mcq_sweep_variant answers for a device of 1 024 SIMDs when
none is there: the MI355X's count).

Per reachable row of SWEEP_TABLE: the row fixes mode, lanes, stream, trace mode, early stop, exchange and the line-counter flag; N
(and, for full_3d, Q = N^2 or another count) is scanned over everything the library takes at the typical chain count, and the smallest
and the largest N that select the row become cases.  A row nothing small selects gets the smallest chain count that selects it, by
bisection.  Schedule, init mode, patience and seed of a case are walked through fixed lists until the oracle's result has what
tests/variant_cases.broken_conditions asks for, and the naive and the fast oracle agree."""
import sys

import numpy as np

from oracle import oracle
from tests import util
from tests import variant_cases as vc

abi = vc.abi
SCHEDS = ("LIN", "EXP", "LOG", "SIN", "CONST")
PATIENT = (("COLD", 25), ("CONST", 40), ("LIN", 40), ("COLD", 60), ("WARM", 15), ("LIN", 90), ("COLD", 12), ("EXP", 25), ("WARM", 40), ("COLD", 120), ("LIN", 200), ("WARM", 6),
           ("SIN", 300), ("EXP", 290), ("LOG", 250), ("SIN", 200), ("EXP", 150), ("LIN", 300))  # (the large ones: the boards of three and four cells, done early)
INITS = ("random", "latin", "klarner")
STEPS = (333, 389, 470, 315)
LARGE_STEPS = 301


def typical_chains(row):
    return 5 if row[12] else 2 * (64 // row[1]) + 1


def args_of(row, N, chains, Q=None, exch=None, sched=("LIN",), steps=333, patience=25):
    return dict(mode="full_3d" if row[0] else "board", N=N, chains=chains, steps=steps, init="random", sched=sched, lanes=row[1], seed=0,
                patience=patience if row[2] else None, trace="reduced" if row[4] else True, rng="philox" if row[5] else "mt19937", flags="CNT" if row[11] else 0,
                Q=Q, exch=exch)


def realise(a):
    """The case of a set of arguments whose schedules and flags are still names."""
    return vc.case(**dict(a, sched=[getattr(vc, s) for s in a["sched"]], flags=vc.CNT if a["flags"] else 0))


def selects(row, a):
    try:
        return vc.variant_of(vc.build(realise(a))[0]) == row
    except ValueError:  # what make_params or validate() refuses
        return False


def sizes(row, chains, exch=None):
    """{N: Q} of the boards / cubes that select the row at this chain count: Q = N^2 (None) where that does, another count where only that does."""
    out = {}
    top = abi.MAX_N if row[0] else abi.MAX_N_BOARD
    for N in range(abi.MIN_N, top + 1):
        other = N * N + 13
        for Q in (None, other) if row[0] and other < min(N**3, 32768) else (None,):
            if N not in out and selects(row, args_of(row, N, chains, Q=Q, exch=exch)):
                out[N] = Q
    return out


def ends_of(ns):
    """The smallest and the largest N of a row, and N = 3 besides N = 2: there no move changes the energy."""
    return sorted({min(ns), max(ns)} | ({3} if min(ns) == 2 and 3 in ns else set()))


def smallest_count(row, N, Q, hi=65537):
    lo = typical_chains(row)  # does not select
    assert selects(row, args_of(row, N, hi, Q=Q)) and not selects(row, args_of(row, N, lo, Q=Q))
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if selects(row, args_of(row, N, mid, Q=Q)) else (mid, hi)
    return hi


def settle(row, a, k):
    """Walk schedule / init / patience / seed until the oracle's result of the case holds the conditions; k: the case's number."""
    large = a["chains"] > vc.MAX_CHAINS
    for t in range(72):
        b = dict(a, seed=1000 * (k + 1) + 7 * t)
        n_sets = len(a["sched"])
        if row[2]:
            s, pat = PATIENT[t % len(PATIENT)]
            b.update(sched=tuple([s] + [SCHEDS[(k + t + u) % 5] for u in range(1, n_sets)]), patience=pat)
        else:
            b.update(sched=tuple(SCHEDS[(k + t + u) % 5] for u in range(n_sets)))
        if n_sets > 1:
            b.update(inits=tuple(INITS[(k + t + u) % 3] for u in range(n_sets)))
            b["init"] = b["inits"][0]
        else:
            b["init"] = "random" if a["Q"] is not None else INITS[(k + t) % 3]
        c = realise(b)
        try:
            p, seeds = vc.build(c)
            if vc.variant_of(p) != row:
                continue
            fast = oracle.run(p, seeds, n_threads=8, fast=True)
            if vc.broken_conditions(row, c, fast):
                continue
            if not large:
                util.assert_results_equal(oracle.run(p, seeds, n_threads=8), fast, str(c))
        except (ValueError, RuntimeError):  # an init mode the size does not have
            continue
        return b
    raise SystemExit(f"no case for {row} from {a}")


def fmt(row, b):
    words = [repr(b["mode"])] + [f"{f}={b[f]!r}" for f in ("N", "chains", "steps", "init")]
    words.append("sched=(" + ", ".join(b["sched"]) + ("," if len(b["sched"]) == 1 else "") + ")")
    words += [f"lanes={b['lanes']}", f"seed={b['seed']}"]
    for f, default in (("patience", None), ("trace", True), ("rng", "mt19937"), ("flags", 0), ("Q", None), ("exch", None), ("inits", None)):
        if b.get(f, default) != default:
            words.append(f"{f}={b[f]}" if f == "flags" else f"{f}={b[f]!r}")
    return f"    ({row}, case({', '.join(words)})),".replace("'", '"')


def derive():
    lines, k, large = [], 0, {}
    for row in vc.reachable_rows():
        G, red, exch, slim = row[1], row[4], row[7], row[10]
        drafts = []
        if exch:
            # whole ladders: the widest the lane count takes (16 rungs at most) in three ladders (five at two lanes: half a wavefront stays idle),
            # and ladders of two over two wavefronts and a part of a third; both at both ends of the row's N
            R = min(16, 64 // G)
            shapes = (((7, R, 0.7, 1.4), R * (5 if G == 2 else 3)), ((3, 2, 0.7, 1.4), 2 * (64 // G) + 2))
            for e, chains in shapes:
                ns = sizes(row, chains, exch=e)
                for N in ends_of(ns):
                    drafts.append(args_of(row, N, chains, Q=ns[N], exch=e))
        else:
            chains = typical_chains(row)
            ns = sizes(row, chains)
            if not ns:  # only a launch beyond a "roomy" threshold: the smallest count that selects the row, at each end of N
                ns = sizes(row, 65537)
                counts = {N: smallest_count(row, N, ns[N]) for N in (min(ns), max(ns))}
                assert len(set(counts.values())) == 1
                chains = large[row] = counts[min(ns)]
            ends = ends_of(ns)
            for i, N in enumerate(ends):
                a = args_of(row, N, chains, Q=ns[N])
                if red and chains <= vc.MAX_CHAINS and i == 0 and ns[N] is None:  # two schedule sets at the small end (whole wavefronts: a wavefront belongs to one set)
                    sets = dict(a, chains=2 * (32 if G == 2 else 16), sched=("LIN", "SIN"))
                    if selects(row, sets):
                        drafts.append(sets)
                        if len(ends) > 1:
                            continue
                drafts.append(a)
            if slim and not any(d["Q"] for d in drafts):  # a queen count other than N^2 where the row takes one
                other = sizes(row, chains)
                other = {N: N * N + 13 for N in other if selects(row, args_of(row, N, chains, Q=N * N + 13))}
                if other:
                    drafts.append(args_of(row, max(other), chains, Q=other[max(other)]))
        assert drafts, row
        for a in drafts:
            a["steps"] = LARGE_STEPS if a["chains"] > vc.MAX_CHAINS else STEPS[k % len(STEPS)]
            lines.append(fmt(row, settle(row, a, k)))
            k += 1
        print(f"{row}: {len(drafts)} cases", file=sys.stderr)
    return lines, large


def main():
    assert vc.mcq_amd._lib.lib().mcq_device_simds() == 1024
    lines, large = derive()
    print("\n".join(lines))
    print("LARGE_ROWS:", large, file=sys.stderr)
    assert large == vc.LARGE_ROWS, "tests/variant_cases.LARGE_ROWS is not what the bisection finds"
    if "--write" in sys.argv[1:]:
        path = vc.__file__
        src = open(path).read()
        head, rest = src.split("    # --- table begin (tools/derive_variant_cases.py --write)\n")
        _, tail = rest.split("    # --- table end\n")
        open(path, "w").write(head + "    # --- table begin (tools/derive_variant_cases.py --write)\n" + "\n".join(lines) + "\n    # --- table end\n" + tail)


if __name__ == "__main__":
    main()
