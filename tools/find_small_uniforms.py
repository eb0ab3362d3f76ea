"""Search the seeds of the searched chains of tests/accept_range_util.py: chains whose stream holds, as the uniform of a step with dE > 0,
a value so small (or so near 1) that no seed taken at random shows one within a few hundred steps.  CPU only.

    python tools/find_small_uniforms.py [case ...] [--procs 8]

Per case, in two phases:

  1. the rare tiers (a27 = word >> 5 of 0, of 1 to 3, and of 4 to 63), in parallel over seeds:
       scan    the first words of the seed's stream, as many as a chain of the case draws, for a word below 2048 (oracle.rng_stream,
               either generator); of the words from 128 on, frequent as they are, only every 8th seed's are followed up
       locate  the step whose uniform starts at that word: accept_range_util.step_of_word bisects on the oracle's word count, here under
               the base row
       keep    the seed when that step has dE > 0
     and then, in one process, places the kept seeds in the order of their steps under the row as it grows -- a seed whose chain an
     earlier point of the row has shifted drops out -- until the seven entries of RARE_PLAN for these tiers stand.  The order is the
     case's entry of accept_range_util.ORDER.
  2. the frequent tiers (top, low-3): accept_range_util.craft() runs with a `search` function that tries consecutive seeds under exactly
     the rows the crafting will rebuild.

It prints the entries of accept_range_util.SEARCHED and ORDER per case.  Nothing trusts these literals: the crafting derives step and u again."""
import argparse
import multiprocessing
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import oracle  # noqa: E402
from tests import accept_range_util as ar  # noqa: E402

RARE_TIERS = ("zero", "low-5", "low-4")
N_RARE = sum(1 for e in ar.RARE_PLAN if e[0] in RARE_TIERS)
ROOM = 5  # steps kept free per searched point still to come in the row


def _tier_of(a):
    return next(t for t in RARE_TIERS if ar.TIERS[t][0] <= a < ar.TIERS[t][1])


def _scan_locate(job):
    """[(step, seed, tier)] of the seeds [first, first + count): the rare words that are the uniform of a step with dE > 0 under the base row."""
    name, first, count, n_words = job
    case = ar.CASES_BY_NAME[name]
    base, out = case.base_table()[ar.RARE], []
    for seed in range(first, first + count):
        w = oracle.rng_stream(seed, "u32", n_words, rng=case.rng)
        known = {}
        for j in np.nonzero(w < (2048 if seed % 8 == 0 else 128))[0]:
            s = ar.step_of_word(case, seed, base, int(j), known)
            if s is not None and s >= ar.FIRST_STEP and ar._probe(case, ar._Streams(case.rng), seed, base, s, None)[0] > 0:
                out.append((s, seed, _tier_of(int(w[j]) >> 5)))
    return out


class Finder:
    def __init__(self, case, index, procs):
        self.case, self.procs = case, procs
        self.next_scan = 10_000_000 * (index + 1)  # far from every case's consecutive seeds and from the other cases' scans
        self.next_plain = 1_000_000 * (index + 1)
        self.scanned, self.scan_seconds, self.rare = 0, 0.0, {}
        base = case.base_table()
        self.n_words = int(np.mean([ar.words_after(case, int(s), base[0], case.n_steps - 1) for s in case.seeds(searching=True)[:8]]))
        self.chunk = max(2000 * procs, int(2e10 / self.n_words))  # seeds per round

    def place(self, cands):
        """The kept seeds in the order of their steps, each under the row with the earlier ones placed: {entry: seed} and the order."""
        case, row, after, streams = self.case, self.case.base_table()[ar.RARE], ar.FIRST_STEP, ar._Streams(self.case.rng)
        remaining, placed = list(range(N_RARE)), []
        for _, seed, tier in sorted(cands):
            limit = case.n_steps - 2 - ROOM * (len(ar.RARE_PLAN) - N_RARE + len(remaining) - 1)
            for i in remaining:
                if ar.RARE_PLAN[i][0] == tier:
                    found = ar.small_uniform_step(case, streams, seed, row, *ar.RARE_PLAN[i], after)
                    if found is not None and found[0] <= limit:
                        row[found[0]], after = found[3], found[0] + 1 + ar.GAP
                        placed.append((i, seed))
                        remaining.remove(i)
                        break
            if not remaining:
                break
        return placed, remaining

    def find_rare(self, pool):
        cands = []
        while True:
            t0, per = time.time(), max(1, self.chunk // (4 * self.procs))
            jobs = [(self.case.name, self.next_scan + k * per, per, self.n_words) for k in range(4 * self.procs)]
            for part in pool.map(_scan_locate, jobs):
                cands += part
            self.next_scan += per * len(jobs)
            self.scanned += per * len(jobs)
            self.scan_seconds += time.time() - t0
            placed, remaining = self.place(cands)
            print(f"#   {self.case.name}: {self.scanned} seeds scanned, {len(cands)} kept, entries still open: {remaining}", file=sys.stderr, flush=True)
            if not remaining:
                self.rare = dict(placed)
                return tuple(i for i, _ in placed) + tuple(range(N_RARE, len(ar.RARE_PLAN)))

    def search(self, case, streams, row, entry, after):
        tier, kind, spec = entry
        if tier in RARE_TIERS:
            return self.rare[ar.RARE_PLAN.index(entry)]
        i = ar.RARE_PLAN.index(entry) if entry in ar.RARE_PLAN else len(ar.RARE_PLAN) - 1
        limit = case.n_steps - 2 - ROOM * (len(ar.RARE_PLAN) - 1 - i)
        while True:  # frequent: consecutive seeds, the first that places the point soon
            seed, self.next_plain = self.next_plain, self.next_plain + 1
            found = ar.small_uniform_step(case, streams, seed, row, tier, kind, spec, after)
            if found is not None and found[0] <= min(limit, after + 40):
                return seed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("cases", nargs="*", default=[c.name for c in ar.CASES])
    ap.add_argument("--procs", type=int, default=min(8, os.cpu_count() or 1))
    args = ap.parse_args()
    with multiprocessing.Pool(args.procs) as pool:
        for name in args.cases:
            case = ar.CASES_BY_NAME[name]
            t0 = time.time()
            finder = Finder(case, ar.CASES.index(case), args.procs)
            case.searched, case.order = None, finder.find_rare(pool)
            table, points, seeds = ar.craft(case, search=finder.search)
            n = case.set_chains
            case.searched = tuple([int(seeds[ar.HIGH * n])] + [int(seeds[ar.RARE * n + i]) for i in range(len(ar.RARE_PLAN))])
            ar.check_plan_was_met(case, points)
            print(f'SEARCHED    "{name}": {case.searched},', flush=True)
            if case.order != tuple(range(len(ar.RARE_PLAN))):
                print(f'ORDER       "{name}": {case.order},', flush=True)
            print(f"#   {name}: {finder.scanned} seeds x {finder.n_words} words scanned and located in {finder.scan_seconds:.0f} s on {args.procs} processes, "
                  f"{time.time() - t0:.0f} s in all", file=sys.stderr, flush=True)


if __name__ == "__main__":
    main()
