"""Crafting of beta tables for replica exchange: the pair's uniform next to its swap probability, and a chain's uniform next to its
acceptance probability at beta(step) * ladder[rung] (tests/test_exchange_ties_host.py, tests/test_exchange_ties.py).  It extends
tests/near_tie_util.py, whose header says what a point is and why the distances are the ones they are.

The swap after step s decides by u < exp(x), x = (beta(s) l_t - beta(s) l_{t+1}) (E_a - E_b), a the chain on rung t.  beta(s) is the
caller's, but it also runs step s itself, so E_a - E_b is only known once beta(s) is.  That is a fixed point: run the set's oracle s + 1
steps under the table so far, read E_a - E_b and u (the last two words of a's stream), set beta(s) so that exp(x) stands where it is
wanted, run again; when (E_a - E_b, u) did not move -- step s of neither chain changed its decision or its word count -- the point
stands, otherwise derive beta(s) again from the new values, six rounds at the most.  The walk through the float64 neighbours of beta(s)
evaluates the oracle's own expression in its order.  For a general ladder beta l_t - beta l_{t+1} carries the rounding of both products,
so one ulp of beta may move exp(x) by more than one: a walk that misses its distance hands the point over to the next pair.

A step point under exchange is near_tie_util's, with three differences: the probe runs the chain's whole set (ladders are coupled), the
rung of the chain during step s comes from an s-step run, and the walk evaluates exp(-(beta l_rung) dE).  A chain is asked for a step
point only after it has swapped at least once, and one `count` point per case sits on the very step after an event in which its chain
swapped ("fresh"): a multiplier or a rung from before the swap decides wrongly there.

One table row serves a whole set, so a step carries one point, and both kinds go in step order over one row, each derived under the row
as changed so far.  Nothing here touches a GPU or looks at a result of the code under test: the expected counts are the crafted ones.

Kinds of swap points (signed distance d = position of the probability minus position of u, so d > 0 swaps):
  count  d = +-2, +-3 ulp: counted, on the LOWER chain a alone
  miss   d = +-8 ulp: no tie
  far    probability = u (1 + delta), |delta| = 2^-30 and 2^-12: no tie, decision known

The ladders: no entry and no ratio of neighbours is a float32 number or a power of two, or beta l_a - beta l_b, beta (l_a - l_b) and the
float32 image of the ladder would agree and a point would see nothing.  A geometric ladder from 0.7 gives that.  The two cases listed
with 0.5 .. 2.0 have the float32 numbers 0.5 and 2.0 as their END rungs (every pair still holds an inner rung, which is none); step
points are not placed on a chain while it sits on an end rung of those two.
"""
import math

import numpy as np

import mcq_amd
from oracle import oracle
from tests import near_tie_util as nt

abi = mcq_amd.abi

SWAP_FAR_DELTAS = (2.0 ** -30, -(2.0 ** -30), 2.0 ** -12, -(2.0 ** -12))
ROUNDS = 6


def geometric(R, lo, hi):
    return lo * (hi / lo) ** (np.arange(R) / (R - 1))


def is_float32(x):
    return float(np.float32(x)) == float(x)


class XCase(nt.Case):
    """A near_tie_util.Case under replica exchange: every set holds set_chains / R ladders of R consecutive chains."""

    def __init__(self, name, mode, N, lanes, R, K, ladder=(0.7, 1.4), **kw):
        super().__init__(name, mode, N, lanes, **kw)
        self.R, self.K, self._of = int(R), int(K), None
        self.ladder = np.ascontiguousarray(geometric(self.R, *ladder) if self.R > 2 else ladder, dtype=np.float64)
        assert len(self.ladder) == self.R and self.set_chains % self.R == 0

    def params(self, table, flags=0, n_steps=None, first_step=0, patience="case", trace="case", ladder=None):
        assert first_step == 0, "the pairing of an event follows the step count from 0"
        p = super().params(table, flags=flags, n_steps=n_steps, trace=trace)
        return abi.set_exchange(p, self.K, self.ladder if ladder is None else ladder)

    def one_set(self, t):
        """Set t alone, as a case of its own (the crafting and the host tests run single sets)."""
        sub = XCase(self.name, self.mode, self.N, self.lanes, self.R, self.K, n_sets=1, n_steps=self.n_steps, trace=True, rng=self.rng)
        sub.ladder, sub._of = self.ladder, (self, t)
        return sub

    def seeds(self):
        if self._of is None:
            return super().seeds()
        whole, t = self._of
        return whole.seeds()[t * self.set_chains: (t + 1) * self.set_chains]

    def base_schedules(self):
        return super().base_schedules() if self._of is None else [self._of[0].base_schedules()[self._of[1]]]

    def draws_at_event(self, rung, s):
        """Does the chain on `rung` during step s draw the uniform of a swap after it (the lower chain of a pair)?"""
        if (s + 1) % self.K:
            return False
        return (rung - (s + 1) // self.K) % 2 == 0 and rung + 1 < self.R


# One case per exchange kernel of the MT19937 stream (tests/test_exchange_ties_host.py asserts it), the board's unrolled N = 12 kernel a
# second time without a trace.  The Philox stream has cases of its own below: its stream_words output is 0 by contract, so the place of an
# event's uniform in the stream comes from the oracle's own word count (oracle.run(words=True)), for both generators.
CASES = (
    XCase("x_board6_g2", "board", 6, 2, 16, 3, seed=3100, n_steps=449),
    XCase("x_board6_g4", "board", 6, 4, 16, 1, seed=3200, n_steps=317),
    XCase("x_board12_g4", "board", 12, 4, 4, 5, ladder=(0.5, 2.0), seed=3300, n_steps=395),
    XCase("x_board12_g8", "board", 12, 8, 8, 4, seed=3400, n_steps=351),
    XCase("x_board17_g16", "board", 17, 16, 4, 7, seed=3500, n_steps=470),
    XCase("x_board12_notrace", "board", 12, 0, 16, 2, trace=False, seed=3600, n_steps=341),
    XCase("x_full3d6_g4", "full_3d", 6, 4, 2, 2, ladder=(0.7, 1.3), seed=3700, n_steps=321),
    XCase("x_full3d12_g8", "full_3d", 12, 8, 8, 3, seed=3800, n_steps=338),
    XCase("x_full3d17_g16", "full_3d", 17, 16, 4, 5, ladder=(0.5, 2.0), seed=3900, n_steps=403),
    XCase("x_full3d6_g8", "full_3d", 6, 8, 8, 4, seed=4000, n_steps=309),
)
# One case per exchange kernel of the Philox stream (tests/test_philox_ties_host.py asserts it), with ladders of 2, 4, 8 and 16 rungs among them.
PHILOX_CASES = (
    XCase("px_board6_g2", "board", 6, 2, 16, 3, seed=8100, n_steps=449, rng="philox"),
    XCase("px_board12_g4", "board", 12, 4, 4, 5, ladder=(0.5, 2.0), seed=8200, n_steps=395, rng="philox"),
    XCase("px_board12_g8", "board", 12, 8, 8, 4, seed=8300, n_steps=351, rng="philox"),
    XCase("px_board17_g16", "board", 17, 16, 4, 7, seed=8400, n_steps=470, rng="philox"),
    XCase("px_full3d6_g4", "full_3d", 6, 4, 2, 2, ladder=(0.7, 1.3), seed=8500, n_steps=321, rng="philox"),
    XCase("px_full3d12_g8", "full_3d", 12, 8, 8, 3, seed=8600, n_steps=338, rng="philox"),
    XCase("px_full3d17_g16", "full_3d", 17, 16, 4, 1, seed=8700, n_steps=403, rng="philox"),
)
PHILOX_ROW = {
    "px_board6_g2": (0, 2, 0, 0),
    "px_board12_g4": (0, 4, 0, 0),
    "px_board12_g8": (0, 8, 0, 0),
    "px_board17_g16": (0, 16, 0, 0),
    "px_full3d6_g4": (1, 4, 0, 0),
    "px_full3d12_g8": (1, 8, 0, 0),
    "px_full3d17_g16": (1, 16, 0, 0),
}
CASES_BY_NAME = {c.name: c for c in CASES + PHILOX_CASES}
# the rows of SWEEP_TABLE with EXCH and without PHILOX, as (MODE, G, NT, NC)
EXCHANGE_ROWS = {(0, 2, 0, 0), (0, 4, 3, 12), (0, 4, 0, 0), (0, 8, 0, 0), (0, 16, 0, 0), (1, 4, 0, 0), (1, 8, 3, 12), (1, 8, 0, 0), (1, 16, 0, 0)}
# ... and with PHILOX
PHILOX_EXCHANGE_ROWS = {(0, 2, 0, 0), (0, 4, 0, 0), (0, 8, 0, 0), (0, 16, 0, 0), (1, 4, 0, 0), (1, 8, 0, 0), (1, 16, 0, 0)}


def check_ladder(case):
    lad = [float(x) for x in case.ladder]
    inner = lad if tuple(lad[::len(lad) - 1]) != (0.5, 2.0) else lad[1:-1]
    assert all(b > a for a, b in zip(lad, lad[1:])) and inner
    for x in inner + [b / a for a, b in zip(lad, lad[1:])]:
        assert not is_float32(x) and math.frexp(x)[0] != 0.5, (case.name, x)


def swap_x(beta, lt, lt1, dEab):
    """The oracle's own expression, in its order (run_exchange_group)."""
    return (beta * lt - beta * lt1) * float(dEab)


def _swap_beta_for(spec, lt, lt1, dEab, u):
    """beta with exp(x) at the wanted place next to u, or None."""
    if not ((lt - lt1) * dEab < 0 and nt.X_MIN <= -math.log(u) <= nt.X_MAX):
        return None
    if spec[0] == "rel":
        beta = math.log(u * (1.0 + spec[1])) / ((lt - lt1) * dEab)
        prob = math.exp(swap_x(beta, lt, lt1, dEab))
        if not (prob < 1.0 and abs((prob - u) / u - spec[1]) <= 0.01 * abs(spec[1]) and abs(nt.signed_ulps(prob, u)) > 1000):
            return None
        return beta
    b0 = nt._bits(math.log(u) / ((lt - lt1) * dEab))
    for k in range(2 * nt.WALK + 1):
        beta = nt._from_bits(b0 + ((k + 1) // 2 if k & 1 else -(k // 2)))
        if nt.signed_ulps(math.exp(swap_x(beta, lt, lt1, dEab)), u) == spec[1]:
            return beta
    return None


def step_prob(beta, l, dE):
    return math.exp(-(beta * l) * dE)


def _step_beta_for(spec, l, dE, u):
    x = -math.log(u)
    if dE <= 0 or not (nt.X_MIN <= x <= nt.X_MAX):
        return None
    if spec[0] == "rel":
        beta = -math.log(u * (1.0 + spec[1])) / (dE * l)
        prob = step_prob(beta, l, dE)
        if not (prob < 1.0 and abs((prob - u) / u - spec[1]) <= 0.01 * abs(spec[1]) and abs(nt.signed_ulps(prob, u)) > 1000):
            return None
        return beta
    b0 = nt._bits(x / (dE * l))
    for k in range(2 * nt.WALK + 1):
        beta = nt._from_bits(b0 + ((k + 1) // 2 if k & 1 else -(k // 2)))
        if nt.signed_ulps(step_prob(beta, l, dE), u) == spec[1]:
            return beta
    return None


def _plans(case, t):
    """What set t is asked for: (swap requests, step requests), each in the order it is placed.  A swap request is (kind, spec, again):
    `again` wants the tie on a chain that already holds a swap tie.  A step request is (kind, spec, who): who = "fresh" (the step after
    an event in which the chain swapped), "tied" (a chain that holds a swap tie) or "any"."""
    C, M, F = nt.COUNT_ULPS, nt.MISS_ULPS, SWAP_FAR_DELTAS
    swaps = [("count", ("ulp", C[t % 4]), False), ("miss", ("ulp", M[t % 2]), False), ("count", ("ulp", C[(t + 1) % 4]), True),
             ("far", ("rel", F[t % 4]), False), ("count", ("ulp", C[(t + 2) % 4]), False), ("far", ("rel", F[(t + 2) % 4]), False),
             ("count", ("ulp", C[(t + 3) % 4]), True), ("miss", ("ulp", M[(t + 1) % 2]), False)]
    brackets = [("bracket", ("rel", d), "any") for i, d in enumerate(nt.BRACKET_DELTAS) if i % case.n_sets == t % case.n_sets]
    steps = [brackets[0], ("count", ("ulp", C[(t + 2) % 4]), "fresh"), brackets[1], ("count", ("ulp", C[(t + 3) % 4]), "tied"), brackets[2],
             ("miss", ("ulp", M[t % 2]), "any")] + brackets[3:] + [("count", ("ulp", C[t % 4]), "tied")]
    return swaps, steps


class _SetRuns:
    """Oracle runs of one set under its row, for the crafting."""

    def __init__(self, case, t, row):
        self.sub, self.row, self.streams = case.one_set(t), row, nt._Streams(case.rng)
        self.seeds = self.sub.seeds()
        self.start = np.arange(case.set_chains) % case.R

    def run(self, n, last_beta=None):
        """The first n steps; last_beta replaces beta(n - 1).  n = 0: the start."""
        if n == 0:
            return {"exchange_rung": self.start, "n_exchanges": np.zeros(len(self.start), dtype=np.int64)}
        tab = np.array(self.row[:n], dtype=np.float64).reshape(1, n)
        if last_beta is not None:
            tab[0, n - 1] = last_beta
        return oracle.run(self.sub.params(tab, n_steps=n), self.seeds, states=False, fast=True, words=True)

    def uniform(self, chain, words):
        return nt.uniform_of(*self.streams.pair_before(int(self.seeds[chain]), int(words)))


def _try_swap(case, runs, s, before, request, tied):
    """A swap point of `request` at the event after step s, or None (the row is then as it was).  `before`: the s-step run."""
    kind, spec, again = request
    row, R, n, lad = runs.row, case.R, (s + 1) // case.K, case.ladder
    rung = before["exchange_rung"]
    pairs = []
    for g in range(case.set_chains // R):
        who = {int(rung[g * R + i]): g * R + i for i in range(R)}
        pairs += [(who[t], who[t + 1], t) for t in range(n & 1, R - 1, 2)]
    if again:
        pairs = [pr for pr in pairs if pr[0] in tied]
    if not pairs:
        return None
    saved, first = float(row[s]), runs.run(s + 1)
    for a, b, t in pairs:
        lt, lt1 = float(lad[t]), float(lad[t + 1])
        seen, res = None, first
        for _ in range(ROUNDS):
            now = (int(res["final_energy"][a]) - int(res["final_energy"][b]), runs.uniform(a, res["rng_words"][a]))
            if now == seen:  # beta(s) was derived from these very values, and they stand under it
                beta, (dEab, u) = float(row[s]), now
                prob = math.exp(swap_x(beta, lt, lt1, dEab))
                return {"what": "swap", "chain": a, "partner": b, "t": t, "step": s, "dEab": dEab, "u": u, "beta": beta, "prob": prob, "swap": bool(u < prob),
                        "kind": kind, "ulps": nt.signed_ulps(prob, u), "counts": 1 if kind == "count" else 0, "moved": t != int(runs.start[a])}
            beta = _swap_beta_for(spec, lt, lt1, *now)
            if beta is None:
                break
            row[s], seen = beta, now
            res = runs.run(s + 1)
        row[s] = saved
    return None


def _try_step(case, runs, s, before, request, tied):
    """A step point of `request` at step s, or None."""
    kind, spec, who = request
    if who == "fresh":
        if s == 0 or s % case.K:
            return None
        eligible = np.nonzero(before["n_exchanges"] != runs.run(s - 1)["n_exchanges"])[0]
    else:
        eligible = np.nonzero(before["n_exchanges"] > 0)[0] if who == "any" else sorted(tied)
    eligible = [int(c) for c in eligible if before["n_exchanges"][c] > 0 and not is_float32(case.ladder[int(before["exchange_rung"][c])])]
    if not eligible:
        return None
    probe = runs.run(s + 1, last_beta=0.0)
    first = (5 * s) % case.set_chains  # spread the points over the set's chains
    for c in sorted(eligible, key=lambda c: (c - first) % case.set_chains):
        rung = int(before["exchange_rung"][c])
        assert nt.accept_bit(probe, c, s), "beta = 0 accepts"
        dE = int(probe["energy_hist"][c, s + 1]) - int(probe["energy_hist"][c, s])
        u = runs.uniform(c, int(probe["rng_words"][c]) - (2 if case.draws_at_event(rung, s) else 0))
        l = float(case.ladder[rung])
        beta = _step_beta_for(spec, l, dE, u)
        if beta is not None:
            runs.row[s] = beta
            prob = step_prob(beta, l, dE)
            return {"what": "step", "chain": c, "step": s, "dE": dE, "u": u, "beta": beta, "prob": prob, "accept": bool(u < prob), "kind": kind,
                    "ulps": nt.signed_ulps(prob, u), "counts": 1 if kind == "count" else 0, "rung": rung, "l": l, "fresh": who == "fresh",
                    "swaps_before": int(before["n_exchanges"][c])}
    return None


def craft(case, first_step=2, gap=6):
    """(table [n_sets][n_steps], points): one dict per crafted point, `what` = "swap" or "step", `chain` (index in the launch) the chain
    that counts the tie; a swap point also holds partner, t (a's rung), dEab, swap, moved (a did not start on rung t), a step point what
    near_tie_util's hold plus rung, l, fresh, swaps_before."""
    table, points = case.base_table(), []
    for t in range(case.n_sets):
        runs = _SetRuns(case, t, table[t])
        swaps, steps = _plans(case, t)
        tied = set()  # chains of the set (local index) that hold a swap tie
        rest = first_step  # the next step that may carry a point: the points are spread over the run
        for s in range(first_step, case.n_steps - 1):
            if not swaps and not steps:
                break
            if s < rest:
                continue
            before = runs.run(s)
            pt = None
            if swaps and (s + 1) % case.K == 0:
                for i, rq in enumerate(swaps[:2]):  # a request that waits for a tied chain does not hold up the next one
                    if i and not swaps[0][2]:
                        break
                    pt = _try_swap(case, runs, s, before, rq, tied)
                    if pt:
                        swaps.pop(i)
                        if pt["counts"]:
                            tied.add(pt["chain"])
                        break
            if pt is None and steps and ((s + 1) % case.K or case.K == 1):
                for i, rq in enumerate(steps[:2]):  # likewise for one that waits for a fresh swap or a tied chain
                    if i and steps[0][2] == "any":
                        break
                    pt = _try_step(case, runs, s, before, rq, tied)
                    if pt:
                        steps.pop(i)
                        break
            if pt:
                pt["set"], rest = t, s + 1 + gap
                for k in ("chain", "partner"):
                    if k in pt:
                        pt[k] += t * case.set_chains
                points.append(pt)
    return table, points


_crafted = {}


def crafted(name):
    """craft() of a listed case, once per process: the tests share it and leave it unchanged."""
    if name not in _crafted:
        table, points = craft(CASES_BY_NAME[name])
        table.setflags(write=False)
        _crafted[name] = (table, tuple(points))
    return _crafted[name]


def swap_points(points):
    return [pt for pt in points if pt["what"] == "swap"]


def step_points(points):
    return [pt for pt in points if pt["what"] == "step"]


def check_plan_was_met(case, points):
    """What is asked of an exchange case's points, so that a crafting that quietly places less fails here and not as a weaker test."""
    check_ladder(case)
    sw, st = swap_points(points), step_points(points)
    assert case.n_sets >= 4 and 300 <= case.n_steps <= 470 and case.n_steps % 16 and case.K <= 8
    for t in range(case.n_sets):
        got = (sum(1 for pt in sw if pt["set"] == t), sum(1 for pt in st if pt["set"] == t))
        assert got[0] >= 4 and got[1] >= 6, f"{case.name}: set {t} holds {got[0]} swap points and {got[1]} step points"
    assert len({(pt["set"], pt["step"]) for pt in points}) == len(points), "one point per step of a row"
    for pts, decision in ((sw, "swap"), (st, "accept")):
        ulps = {pt["ulps"] for pt in pts if pt["kind"] in ("count", "miss")}
        assert ulps >= {2, -2, 3, -3, 8, -8}, (case.name, decision, sorted(ulps))
        for pt in pts:
            assert pt["kind"] != "count" or abs(pt["ulps"]) in (2, 3)
            assert pt["kind"] != "miss" or abs(pt["ulps"]) == 8
            assert pt["kind"] not in ("bracket", "far") or abs(pt["ulps"]) > 1000
            assert pt[decision] == (pt["ulps"] > 0) and pt["counts"] == (pt["kind"] == "count")
        assert {pt[decision] for pt in pts if pt["counts"]} == {True, False}, f"{case.name}: the counted {decision} ties hold one decision only"
    far = sorted((pt["prob"] - pt["u"]) / pt["u"] for pt in sw if pt["kind"] == "far")
    assert all(any(abs(g - w) <= 0.02 * abs(w) for g in far) for w in SWAP_FAR_DELTAS), f"{case.name}: far swap points {far}"
    swap_ties, step_ties = (nt.expected_near_ties(case, pts) for pts in (sw, st))
    assert swap_ties.max() >= 2, f"{case.name}: no chain is credited two swap ties"
    assert ((swap_ties > 0) & (step_ties > 0)).any(), f"{case.name}: no chain holds a swap tie and a step tie"
    assert any(pt["moved"] for pt in sw), f"{case.name}: every swap point has its lower chain on the rung it started on"
    assert all(pt["swaps_before"] > 0 and not is_float32(pt["l"]) for pt in st)
    assert any(pt["fresh"] and pt["counts"] for pt in st), f"{case.name}: no counted step point on the step after its chain swapped"
    got = sorted((pt["prob"] - pt["u"]) / pt["u"] for pt in st if pt["kind"] == "bracket")
    want = sorted(nt.BRACKET_DELTAS)
    assert len(got) == len(want) and all(abs(g - w) <= 0.02 * abs(w) for g, w in zip(got, want)), f"{case.name}: bracket points {got}"


def recomputed(case, pt):
    """The decision of a crafted point from (u, beta, energies, ladder) alone, in the oracle's order."""
    if pt["what"] == "swap":
        return pt["u"] < math.exp(swap_x(pt["beta"], float(case.ladder[pt["t"]]), float(case.ladder[pt["t"] + 1]), pt["dEab"]))
    return pt["u"] < step_prob(pt["beta"], pt["l"], pt["dE"])
