"""Crafting of beta tables that put a chain's uniform next to its acceptance probability (tests/test_near_ties_host.py, tests/test_near_ties.py;
on the Philox stream tests/test_philox_ties_host.py, tests/test_philox_ties.py).

A caller's mcq_params.beta_table is followed exactly, the proposal of step s does not depend on beta(s), and the uniform of a step is always
drawn and is the last two words of the step.  So for a chosen (step s, chain c) the CPU oracle, run for s + 1 steps under the table as
crafted so far with beta(s) = 0 (everything is accepted), tells dE = energy_hist[s + 1] - energy_hist[s] and, through the number of words
the chain drew (oracle.run(words=True): the stream_words output is 0 under Philox by contract), the two words of
u = ((w1 >> 5) 2^26 + (w2 >> 6)) 2^-53.  With dE > 0 and x = -ln(u) in [0.05, 1], beta(s) is then walked through the float64
neighbours of x / dE until math.exp(-beta dE) -- glibc's exp, the oracle's -- stands at the wanted SIGNED distance from u; x <= 1 makes one
ulp of beta move exp by less than one ulp, so every distance is hit.  A step that does not qualify hands over to the next step of the chain.
Points are placed in step order: each is derived under the table all earlier points have already changed.

Nothing here touches a GPU, and nothing looks at a result of the code under test: the expected counts are the crafted ones.

Kinds of points (signed distance d = position of the probability minus position of u, so d > 0 accepts):
  count    d = +-2, +-3 ulp: a near tie (|d| <= 4) that stays one, and keeps its decision, while the device's exp and glibc's agree within 1 ulp
  miss     d = +-8 ulp: no tie
  bracket  probability = u (1 + delta) with |delta| from 2^-40 up to 2^-9: inside, at the edge of, and outside the float32 bracket
           (half-width e27 2^-10 + 1/2); never a tie
  behind   (early-stop cases) a +2 ulp tie of a chain at a step behind the one it stopped at: never executed, so it must not count
Distances 0, +-1 and +-4 .. +-7 are left out: there the two exp may legitimately disagree about the count or the decision.
"""
import math
import struct

import numpy as np

import mcq_amd
from oracle import oracle

abi = mcq_amd.abi

SET_CHAINS = 16  # chains_per_set is a multiple of 16: one table row serves 16 chains (one wavefront at 4 lanes per chain)
SET_CHAINS_2 = 32  # ... and of 32 at 2 lanes per chain, where a wavefront holds 32 chains and belongs to one set
COUNT_ULPS = (2, -2, 3, -3)
MISS_ULPS = (8, -8)
# (2^-17 .. 2^-22: around the error of the float32 estimate of exp, where a bracket narrower than that error decides wrongly)
BRACKET_DELTAS = tuple(s * m for m in (2.0 ** -40, 2.0 ** -30, 2.0 ** -22, 2.0 ** -21, 2.0 ** -20, 2.0 ** -19, 2.0 ** -18, 2.0 ** -17, 2.0 ** -16, 2.0 ** -14,
                                       2.0 ** -12, 0.9 * 2.0 ** -10, 1.1 * 2.0 ** -10, 2.0 ** -9) for s in (1.0, -1.0))
X_MIN, X_MAX = 0.05, 1.0
WALK = 400


def _bits(x):
    return struct.unpack("<q", struct.pack("<d", x))[0]


def _from_bits(b):
    return struct.unpack("<d", struct.pack("<q", b))[0]


def signed_ulps(prob, u):
    """Position of `prob` minus position of `u` among the float64 values (both positive and finite)."""
    return _bits(prob) - _bits(u)


def uniform_of(w1, w2):
    """NumPy's random_sample from two 32-bit words: 53 bits, exact in float64."""
    return ((int(w1) >> 5) * 67108864 + (int(w2) >> 6)) / 9007199254740992.0


class Case:
    """One launch: n_sets sets of 16 chains (32 at 2 lanes per chain), each under its own table row."""

    def __init__(self, name, mode, N, lanes, n_sets=4, n_steps=330, trace=True, patience=None, Q=None, seed=1000, rng="mt19937"):
        self.name, self.mode, self.N, self.lanes, self.n_sets, self.n_steps = name, mode, int(N), int(lanes), int(n_sets), int(n_steps)
        self.set_chains = SET_CHAINS_2 if self.lanes == 2 else SET_CHAINS
        self.trace, self.patience, self.Q, self.seed, self.rng = trace, patience, Q, int(seed), rng

    @property
    def n_chains(self):
        return self.n_sets * self.set_chains

    def seeds(self):
        return abi.seeds_for(self.seed, self.n_chains)

    def base_schedules(self):
        """Every set its own mild linear schedule: what the steps nobody crafts run under."""
        return [{"type": "linear_annealing", "beta_start": 0.2 + 0.05 * t, "beta_end": 0.9 + 0.1 * t} for t in range(self.n_sets)]

    def base_table(self):
        return np.ascontiguousarray(np.stack([abi.beta_values(sp, self.n_steps) for sp in self.base_schedules()]))

    def params(self, table, flags=0, n_steps=None, first_step=0, patience="case", trace="case"):
        """The Params block of the launch (or of its steps [first_step, first_step + n_steps)) under `table` ([n_sets][whole run]); the
        block keeps the slice it points to alive."""
        n = self.n_steps if n_steps is None else int(n_steps)
        p = abi.make_params_sets(self.N, n, "random", self.base_schedules(), self.set_chains, mcmc_type=self.mode,
                                 early_stop_patience=self.patience if patience == "case" else patience,
                                 trace=self.trace if trace == "case" else trace, flags=flags, lanes_per_chain=self.lanes, rng=self.rng)
        if self.Q is not None:
            p.n_queens = int(self.Q)
        tab = np.ascontiguousarray(np.asarray(table, dtype=np.float64)[:, first_step: first_step + n])
        assert tab.shape == (self.n_sets, n)
        p._schedules, p.beta_table, p._beta_keepalive = None, tab.ctypes.data, tab
        return p


# the launches the issue lists; `lanes` 0 = the library's default
CASES = (
    Case("board6_g2", "board", 6, 2, seed=1100, n_steps=450),
    Case("board6_g4", "board", 6, 4, seed=1200, n_steps=317),
    Case("board12_g4", "board", 12, 4, seed=1300, n_steps=330),
    Case("board12_g8", "board", 12, 8, seed=1400, n_steps=351),
    Case("board12_g16", "board", 12, 16, seed=1500, n_steps=470),
    Case("board17_g8", "board", 17, 8, seed=1600, n_steps=333),
    Case("board40", "board", 40, 0, seed=1700, n_steps=305),
    Case("board12_notrace", "board", 12, 0, trace=False, seed=1800, n_steps=340),
    Case("board12_reduced", "board", 12, 0, trace="reduced", seed=1900, n_steps=345),
    Case("board12_patience", "board", 12, 0, patience=60, seed=2000, n_steps=400),
    Case("full3d6_g8", "full_3d", 6, 8, seed=2100, n_steps=321),
    Case("full3d10_g4", "full_3d", 10, 4, seed=2200, n_steps=338),
    Case("full3d6_q20", "full_3d", 6, 0, Q=20, seed=2300, n_steps=310),
    Case("full3d40", "full_3d", 40, 0, seed=2400, n_steps=300),
)
# The same on the Philox stream, one launch per plain row of SWEEP_TABLE with PHILOX (tests/test_philox_ties_host.py asserts it): the sizes
# are the ones that select the row -- N = 9 and 12 for the board's unrolled candidate loops at 4 lanes and full_3d's at 8, N = 17 for the
# run-time loop at 8 and 16 lanes -- and PATIENCE x REDUCED is run in all four combinations, which no MT19937 case does.  A Philox run
# cannot be resumed, so none of these is cut into segments.
PHILOX_CASES = (
    Case("p_board6_g2", "board", 6, 2, seed=5100, n_steps=450, rng="philox"),
    Case("p_board6_g2_patience", "board", 6, 2, patience=60, seed=5200, n_steps=421, rng="philox"),
    Case("p_board6_g2_reduced", "board", 6, 2, trace="reduced", seed=5300, n_steps=443, rng="philox"),
    Case("p_board6_g2_patience_reduced", "board", 6, 2, patience=60, trace="reduced", seed=5400, n_steps=430, rng="philox"),
    Case("p_board6_g4", "board", 6, 4, seed=5500, n_steps=317, rng="philox"),
    Case("p_board6_g4_patience", "board", 6, 4, patience=60, seed=5600, n_steps=400, rng="philox"),
    Case("p_board6_g4_reduced", "board", 6, 4, trace="reduced", seed=5700, n_steps=345, rng="philox"),
    Case("p_board6_g4_patience_reduced", "board", 6, 4, patience=60, trace="reduced", seed=5800, n_steps=389, rng="philox"),
    Case("p_board9_g4", "board", 9, 4, seed=5900, n_steps=325, rng="philox"),
    Case("p_board12_g4", "board", 12, 4, seed=6000, n_steps=330, rng="philox"),
    Case("p_board17_g8", "board", 17, 8, seed=6100, n_steps=333, rng="philox"),
    Case("p_board12_g8_patience", "board", 12, 8, patience=60, seed=6200, n_steps=400, rng="philox"),
    Case("p_board12_g8_reduced", "board", 12, 8, trace="reduced", seed=6300, n_steps=351, rng="philox"),
    Case("p_board17_g8_patience_reduced", "board", 17, 8, patience=40, trace="reduced", seed=6400, n_steps=410, rng="philox"),
    Case("p_board17_g16", "board", 17, 16, seed=6500, n_steps=470, rng="philox"),
    Case("p_board12_g16_patience", "board", 12, 16, patience=60, seed=6601, n_steps=405, rng="philox"),
    Case("p_board17_g16_reduced", "board", 17, 16, trace="reduced", seed=6700, n_steps=341, rng="philox"),
    Case("p_board12_g16_patience_reduced", "board", 12, 16, patience=60, trace="reduced", seed=6801, n_steps=395, rng="philox"),
    Case("p_full3d6_g4", "full_3d", 6, 4, seed=6900, n_steps=321, rng="philox"),
    Case("p_full3d6_g4_reduced", "full_3d", 6, 4, trace="reduced", seed=7000, n_steps=338, rng="philox"),
    Case("p_full3d9_g8", "full_3d", 9, 8, seed=7100, n_steps=329, rng="philox"),
    Case("p_full3d12_g8", "full_3d", 12, 8, seed=7200, n_steps=310, rng="philox"),
    Case("p_full3d6_g8", "full_3d", 6, 8, seed=7300, n_steps=315, rng="philox"),
    Case("p_full3d17_g8_reduced", "full_3d", 17, 8, trace="reduced", seed=7400, n_steps=305, rng="philox"),
    Case("p_full3d17_g16", "full_3d", 17, 16, seed=7500, n_steps=307, rng="philox"),
    Case("p_full3d6_g16_reduced", "full_3d", 6, 16, trace="reduced", seed=7600, n_steps=333, rng="philox"),
)
# the plain rows of SWEEP_TABLE with PHILOX, as (MODE, G, PATIENCE, NT, REDUCED, NC)
PHILOX_ROWS = ({(0, G, P, 0, R, 0) for G in (2, 4, 8, 16) for P in (0, 1) for R in (0, 1)} | {(0, 4, 0, 3, 0, 0), (0, 4, 0, 3, 0, 12)} |
               {(1, 4, 0, 0, 0, 0), (1, 4, 0, 0, 1, 0), (1, 8, 0, 3, 0, 0), (1, 8, 0, 3, 0, 12), (1, 8, 0, 0, 0, 0), (1, 8, 0, 0, 1, 0), (1, 16, 0, 0, 0, 0),
                (1, 16, 0, 0, 1, 0)})
# the row each of them selects (asserted against the library's own selection on the CPU and on the device)
PHILOX_ROW = {
    "p_board6_g2": (0, 2, 0, 0, 0, 0),
    "p_board6_g2_patience": (0, 2, 1, 0, 0, 0),
    "p_board6_g2_reduced": (0, 2, 0, 0, 1, 0),
    "p_board6_g2_patience_reduced": (0, 2, 1, 0, 1, 0),
    "p_board6_g4": (0, 4, 0, 0, 0, 0),
    "p_board6_g4_patience": (0, 4, 1, 0, 0, 0),
    "p_board6_g4_reduced": (0, 4, 0, 0, 1, 0),
    "p_board6_g4_patience_reduced": (0, 4, 1, 0, 1, 0),
    "p_board9_g4": (0, 4, 0, 3, 0, 0),
    "p_board12_g4": (0, 4, 0, 3, 0, 12),
    "p_board17_g8": (0, 8, 0, 0, 0, 0),
    "p_board12_g8_patience": (0, 8, 1, 0, 0, 0),
    "p_board12_g8_reduced": (0, 8, 0, 0, 1, 0),
    "p_board17_g8_patience_reduced": (0, 8, 1, 0, 1, 0),
    "p_board17_g16": (0, 16, 0, 0, 0, 0),
    "p_board12_g16_patience": (0, 16, 1, 0, 0, 0),
    "p_board17_g16_reduced": (0, 16, 0, 0, 1, 0),
    "p_board12_g16_patience_reduced": (0, 16, 1, 0, 1, 0),
    "p_full3d6_g4": (1, 4, 0, 0, 0, 0),
    "p_full3d6_g4_reduced": (1, 4, 0, 0, 1, 0),
    "p_full3d9_g8": (1, 8, 0, 3, 0, 0),
    "p_full3d12_g8": (1, 8, 0, 3, 0, 12),
    "p_full3d6_g8": (1, 8, 0, 0, 0, 0),
    "p_full3d17_g8_reduced": (1, 8, 0, 0, 1, 0),
    "p_full3d17_g16": (1, 16, 0, 0, 0, 0),
    "p_full3d6_g16_reduced": (1, 16, 0, 0, 1, 0),
}
CASES_BY_NAME = {c.name: c for c in CASES + PHILOX_CASES}
SEGMENT_CASES = ("board12_g4", "full3d6_g8")


class _Streams:
    """The raw 32-bit words of each seed's stream (MT19937 or Philox), grown on demand."""

    def __init__(self, rng="mt19937"):
        self.words, self.rng = {}, rng

    def pair_before(self, seed, n_words):
        have = self.words.get(seed)
        if have is None or len(have) < n_words:
            have = oracle.rng_stream(seed, "u32", max(int(n_words) + 4096, 2 * (0 if have is None else len(have))), rng=self.rng)
            self.words[seed] = have
        return int(have[n_words - 2]), int(have[n_words - 1])


def _probe(case, streams, seed, row, s, patience):
    """Chain `seed` under row[:s] and beta(s) = 0: (dE, u) of step s, or None when the chain does not execute step s as a step that appends
    its entry (it stopped early)."""
    tab = np.ascontiguousarray(row[: s + 1]).reshape(1, s + 1).copy()
    tab[0, s] = 0.0
    p = abi.make_params(case.N, s + 1, "random", case.base_schedules()[0], 1, mcmc_type=case.mode, early_stop_patience=patience, Q=case.Q, rng=case.rng)
    p._schedules, p.beta_table = None, tab.ctypes.data
    res = oracle.run(p, np.array([seed], dtype=np.uint32), states=False, words=True)
    if int(res["hist_len"][0]) != s + 2:
        return None
    assert (int(res["accept_bits"][0, s >> 6]) >> (s & 63)) & 1, "beta = 0 accepts"
    dE = int(res["energy_hist"][0, s + 1]) - int(res["energy_hist"][0, s])
    return dE, uniform_of(*streams.pair_before(int(seed), int(res["rng_words"][0])))


def _beta_for(spec, dE, u):
    """beta with exp(-beta dE) at the wanted place next to u, or None.  spec: ("ulp", d) or ("rel", delta)."""
    x = -math.log(u)
    if dE <= 0 or not (X_MIN <= x <= X_MAX):
        return None
    if spec[0] == "rel":
        beta = -math.log(u * (1.0 + spec[1])) / dE
        prob = math.exp(-beta * dE)
        rel = (prob - u) / u
        if not (prob < 1.0 and abs(rel - spec[1]) <= 0.01 * abs(spec[1]) and abs(signed_ulps(prob, u)) > 1000):
            return None
        return beta
    b0 = _bits(x / dE)
    for k in range(2 * WALK + 1):
        beta = _from_bits(b0 + ((k + 1) // 2 if k & 1 else -(k // 2)))
        if signed_ulps(math.exp(-beta * dE), u) == spec[1]:
            return beta
    return None


def _plan_for_set(case, t):
    """The points set t is asked for, in step order: a tie for each of its chains (so that every lane group of a wavefront ties, at
    every lane count), two more for one chain (it ties three times: the count adds up), and among them the near misses and this set's
    share of the bracket points.  An early-stop case asks for fewer: its chains leave."""
    n = case.set_chains
    ties = [("count", ("ulp", COUNT_ULPS[(t + i) % 4]), (5 * t + i) % n) for i in range(n)]
    thrice = ties[1][2]
    ties.insert(2, ("count", ("ulp", COUNT_ULPS[(t + 1) % 4]), thrice))
    ties.insert(3, ("count", ("ulp", COUNT_ULPS[(t + 2) % 4]), thrice))
    others = [("miss", ("ulp", d), (3 * t + 7 * i + 2) % n) for i, d in enumerate(MISS_ULPS)]
    others += [("bracket", ("rel", d), (t + 3 * i) % n) for i, d in enumerate(BRACKET_DELTAS) if i % case.n_sets == t % case.n_sets]
    if case.patience is not None:
        ties, others = ties[:8], others[:5]
    plan, j = [], 0
    for i, tie in enumerate(ties):  # interleaved: a tie, then now and then one of the others
        plan.append(tie)
        if j < len(others) and (i % 2 == 1 or len(ties) - i <= len(others) - j):
            plan.append(others[j])
            j += 1
    return plan + others[j:]


def craft(case, first_step=6, gap=4):
    """(table [n_sets][n_steps], points): the case's base table with beta rewritten at the crafted steps, and one dict per crafted point --
    set, chain (index in the launch), step, dE, u, beta, prob (math.exp(-beta dE)), accept (u < prob), kind, ulps (signed, as measured),
    counts (1 where the oracle and the kernel must count a near tie)."""
    table = case.base_table()
    seeds, streams, points = case.seeds(), _Streams(case.rng), []
    for t in range(case.n_sets):
        row, s = table[t], first_step + t
        for kind, spec, pos in _plan_for_set(case, t):
            placed = False
            for turn in range(case.set_chains):  # a chain that has stopped early hands over to its neighbour
                c = t * case.set_chains + (pos + turn) % case.set_chains
                while s < case.n_steps - 1:
                    probe = _probe(case, streams, seeds[c], row, s, case.patience)
                    if probe is None:
                        break
                    beta = _beta_for(spec, *probe)
                    if beta is not None:
                        placed = True
                        break
                    s += 1
                if placed or s >= case.n_steps - 1:
                    break
            if not placed:
                break
            row[s] = beta
            points.append(_point(t, c, s, probe[0], probe[1], beta, kind, 1 if kind == "count" else 0))
            s += 1 + gap
        if case.patience is not None:
            points += _behind_the_stop(case, streams, seeds, table, t, s)
    return table, points


def _point(t, c, s, dE, u, beta, kind, counts):
    prob = math.exp(-beta * dE)
    return {"set": t, "chain": int(c), "step": int(s), "dE": int(dE), "u": u, "beta": beta, "prob": prob, "accept": bool(u < prob), "kind": kind,
            "ulps": signed_ulps(prob, u), "counts": counts}


def _behind_the_stop(case, streams, seeds, table, t, s):
    """A +2 ulp tie for a chain of set t at a step behind its stop (found without early stopping, where the chain goes on): the step is
    never executed under the case's patience."""
    n = case.set_chains
    sub = Case("set", case.mode, case.N, case.lanes, n_sets=1, n_steps=case.n_steps, patience=case.patience, seed=int(seeds[t * n]), rng=case.rng)
    res = oracle.run(sub.params(table[t: t + 1]), seeds[t * n: (t + 1) * n], states=False)
    stopped = [r for r in range(n) if int(res["steps_executed"][r]) <= s]
    if not stopped:
        return []
    c, row = t * n + stopped[0], table[t]
    while s < case.n_steps - 1:
        probe = _probe(case, streams, seeds[c], row, s, None)
        beta = _beta_for(("ulp", 2), *probe)
        if beta is not None:
            row[s] = beta
            return [_point(t, c, s, probe[0], probe[1], beta, "behind", 0)]
        s += 1
    return []


_crafted = {}


def crafted(name):
    """craft() of a listed case, once per process: the tests share it and leave it unchanged."""
    if name not in _crafted:
        table, points = craft(CASES_BY_NAME[name])
        table.setflags(write=False)
        _crafted[name] = (table, tuple(points))
    return _crafted[name]


def expected_near_ties(case, points):
    want = np.zeros(case.n_chains, dtype=np.int64)
    for pt in points:
        want[pt["chain"]] += pt["counts"]
    return want


def kinds(points):
    out = {}
    for pt in points:
        out[pt["kind"]] = out.get(pt["kind"], 0) + 1
    return out


def check_plan_was_met(case, points):
    """What the issue asks of a case's points, so that a crafting that quietly places less fails here and not as a weaker test."""
    ties = expected_near_ties(case, points)
    per_set = [sum(1 for pt in points if pt["set"] == t) for t in range(case.n_sets)]
    assert case.n_sets >= 4 and 300 <= case.n_steps <= 470 and min(per_set) >= 6, (case.name, per_set)
    assert ties.sum() > 0 and ties.max() >= 3, f"{case.name}: no chain ties three times"
    ulps = {pt["ulps"] for pt in points if pt["kind"] in ("count", "miss")}
    assert ulps >= {2, -2, 3, -3, 8, -8}, (case.name, sorted(ulps))
    for pt in points:
        assert pt["kind"] != "count" or abs(pt["ulps"]) in (2, 3)
        assert pt["kind"] != "miss" or abs(pt["ulps"]) == 8
        assert pt["kind"] != "bracket" or abs(pt["ulps"]) > 1000
        assert pt["accept"] == (pt["ulps"] > 0)
    for d in (1, -1):
        assert {pt["accept"] for pt in points if pt["kind"] == "count" and pt["ulps"] * d > 0} == {d > 0}
    if case.patience is None:
        positions = {pt["chain"] % case.set_chains for pt in points if pt["counts"]}
        assert positions == set(range(case.set_chains)), f"{case.name}: chains {sorted(set(range(case.set_chains)) - positions)} of a set never tie"
        got = sorted((pt["prob"] - pt["u"]) / pt["u"] for pt in points if pt["kind"] == "bracket")
        want = sorted(BRACKET_DELTAS)
        assert len(got) == len(want) and all(abs(g - w) <= 0.02 * abs(w) for g, w in zip(got, want)), f"{case.name}: bracket points {got}"
    else:
        assert any(pt["kind"] == "behind" for pt in points), f"{case.name}: no point behind a chain's stop"


LOCATOR_WORDS = 1 << 16  # of a stream that the bisection locator searches: several times what a chain of these cases draws


def locate_by_bisection(case, table, chain, step):
    """The place of step `step`'s uniform in the chain's stream, found WITHOUT any count of the words drawn: (words, u, pairs) -- the
    number of words of the stream up to and including the uniform, the uniform, and how many consecutive word pairs of the stream's first
    LOCATOR_WORDS words fell into the bracket (the caller asserts 1).  The step must have dE > 0.

    The accept bit of step s under the row so far and beta(s) = b is u < exp(-b dE): true at b = 0, false at b = 64 (exp < 2^-92 < any
    u > 0), and monotone in b as far as glibc's exp is.  Bisecting over the float64 values of b (62 one-chain oracle runs) ends at two
    neighbours b_acc < b_rej with exp(-b_rej dE) <= u < exp(-b_acc dE); for x = b dE <= 1 one ulp of b moves exp by less than one ulp,
    so that interval holds one or two float64 values, and one word pair of a stream of 2^16 words falls into it by chance once in 2^36."""
    t, seed = chain // case.set_chains, int(case.seeds()[chain])
    row = np.array(table[t, : step + 1], dtype=np.float64).reshape(1, step + 1)
    p = abi.make_params(case.N, step + 1, "random", case.base_schedules()[0], 1, mcmc_type=case.mode, Q=case.Q, rng=case.rng)
    p._schedules, p.beta_table = None, row.ctypes.data

    def run(b):
        row[0, step] = b
        return oracle.run(p, np.array([seed], dtype=np.uint32), states=False)

    free = run(0.0)
    dE = int(free["energy_hist"][0, step + 1]) - int(free["energy_hist"][0, step])
    assert accept_bit(free, 0, step) == 1 and dE > 0 and accept_bit(run(64.0), 0, step) == 0
    lo, hi = _bits(0.0), _bits(64.0)  # accepted at lo, rejected at hi
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if accept_bit(run(_from_bits(mid)), 0, step):
            lo = mid
        else:
            hi = mid
    u_min, u_max = math.exp(-_from_bits(hi) * dE), math.exp(-_from_bits(lo) * dE)  # u_min <= u < u_max
    w = oracle.rng_stream(seed, "u32", LOCATOR_WORDS, rng=case.rng).astype(np.uint64)
    us = ((w[:-1] >> np.uint64(5)) * np.uint64(67108864) + (w[1:] >> np.uint64(6))).astype(np.float64) / 9007199254740992.0  # exact: below 2^53
    inside = np.nonzero((us >= u_min) & (us < u_max))[0]
    return (int(inside[0]) + 2 if len(inside) else 0), (float(us[inside[0]]) if len(inside) else None), len(inside)


def reduced_from_trace(res, n_steps, n_sets):
    """What the reduced trace holds (include/mcq.h: step_sum, step_sumsq, step_accepted, step_count per schedule set), from a full trace:
    the oracle writes no reduced trace of its own."""
    L, ex = res["hist_len"].astype(np.int64), res["steps_executed"].astype(np.int64)
    h = res["energy_hist"][:, : n_steps + 1].astype(np.int64)
    valid = np.arange(n_steps + 1)[None, :] < L[:, None]
    hv = np.where(valid, h, 0)
    bits = np.unpackbits(np.ascontiguousarray(res["accept_bits"]).view(np.uint8), axis=1, bitorder="little")[:, :n_steps].astype(np.int64)
    bits *= np.arange(n_steps)[None, :] < ex[:, None]
    acc = np.concatenate([np.zeros((len(L), 1), dtype=np.int64), bits], axis=1)
    per_set = lambda a: a.reshape(n_sets, -1, n_steps + 1).sum(axis=1)  # noqa: E731
    return {"step_sum": per_set(hv), "step_sumsq": per_set(hv * hv), "step_accepted": per_set(acc), "step_count": per_set(valid.astype(np.int64))}


def accept_bit(res, chain, step):
    return (int(res["accept_bits"][chain, step >> 6]) >> (step & 63)) & 1


def _swap_point_behind(points, chain, step):
    """The last crafted swap point (tests/exchange_tie_util.py) in front of `step` in which `chain` took part, described -- a swap that
    went the other way shows in the histories only at a later step of one of the two chains."""
    mine = [pt for pt in points if pt.get("what") == "swap" and chain in (pt["chain"], pt["partner"]) and (step is None or pt["step"] < step)]
    if not mine:
        return "no crafted swap point of that chain in front of it"
    pt = max(mine, key=lambda pt: pt["step"])
    return (f"the last crafted swap point of that chain in front of it: after step {pt['step']}, {pt['kind']} ({pt['ulps']:+d} ulp), chains {pt['chain']} (rung "
            f"{pt['t']}, counts the tie) and {pt['partner']}, E_a - E_b {pt['dEab']}, u {pt['u']!r}, beta {pt['beta']!r}, swap {pt['swap']}")


def first_difference(got, want, points, trace=True):
    """Where two results part, for a failure message: the first (chain, step) whose history entry or accept bit differs (full trace) or the
    first chain whose summary differs, and what was crafted there; under replica exchange also the crafted swap point behind it."""
    at = {(pt["chain"], pt["step"]): pt for pt in points if pt.get("what") != "swap"}
    swaps = any(pt.get("what") == "swap" for pt in points)
    if trace is True:
        best = None
        for r in range(len(want["hist_len"])):
            L = int(want["hist_len"][r])
            for s in range(L - 1):
                if int(got["energy_hist"][r, s + 1]) != int(want["energy_hist"][r, s + 1]) or accept_bit(got, r, s) != accept_bit(want, r, s):
                    if best is None or s < best[1]:
                        best = (r, s)
                    break
        if best is not None:
            pt = at.get(best)
            return (f"first difference at chain {best[0]}, step {best[1]}: " +
                    (f"a crafted {pt['kind']} point ({pt['ulps']:+d} ulp, dE {pt['dE']}, u {pt['u']!r}, beta {pt['beta']!r})" if pt else "not a crafted point") +
                    (f"; {_swap_point_behind(points, best[0], best[1])}" if swaps else ""))
    fields = ("near_ties", "n_accepted", "final_energy", "best_energy", "steps_to_best", "hist_len", "stream_words") + (("exchange_rung", "n_exchanges") if swaps else ())
    for r in range(len(want["near_ties"])):
        for k in fields:
            if int(got[k][r]) != int(want[k][r]):
                mine = [(pt["step"], pt.get("what", "step"), pt["kind"], pt["ulps"]) for pt in points if r in (pt["chain"], pt.get("partner"))]
                return f"first differing chain {r}: {k} {int(got[k][r])} != {int(want[k][r])}; crafted (step, what, kind, ulp) of that chain: {mine}"
    return "no difference in histories, accept bits or summaries"
