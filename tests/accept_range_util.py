"""Crafting of beta tables that try the accept decision over the whole range of x = beta dE (tests/test_accept_range_host.py,
tests/test_accept_range.py): probabilities next to 1, probabilities so small that the 1/2 of the float32 bracket's half-width
w = e27 2^-10 + 1/2 is all of it, negative beta, and beta values that are no ordinary numbers.  It builds on tests/near_tie_util.py (whose
cases, plans and bounds hold x to [0.05, 1]) and changes nothing there.

Nothing here touches a GPU or looks at a result of the code under test.  The truth of every crafted point is u < math.exp(-beta dE), glibc's
exp, cross-checked per point against decimal arithmetic at 60 digits (check_against_decimal); the truth of a special beta value is the
reference's rule u < min(1.0, exp(-beta dE)) evaluated in Python (rule).

A launch has five sets of 16 chains (32 at 2 lanes per chain), each under its own table row:
  high     x in [2^-12, 0.05): ties (+-2, +-3 ulp), near misses (+-8) and relative distances |delta| <= x / 2; its first point, on a searched
           chain, has x < 2^-9
  low      x in (1, 4] and (4, 9]: relative distances inside, at the edge of and outside the bracket
  rare     eleven searched chains whose stream holds a uniform below 2^-13: a27 = the top 27 bits of u in [300, 16000), [4, 64), [1, 4), and 0
  negative a base row from -0.2 to -0.9; points on steps with dE < 0 (beta = x / dE < 0): ties, near misses and relative distances
  special  twelve beta values (zeros, NaN, infinities, denormals, values whose float32 image c32 underflows or overflows) at twelve steps

Kinds of points (never ties unless stated: at least 1000 ulp from u):
  count, miss  +-2, +-3 and +-8 ulp, as in near_tie_util (ties and near misses); only where x <= 1
  rel          prob = u (1 + delta)
  abs          prob = u + eta 2^-27
  bias         an abs point with eta = +-0.05 that float32 arithmetic without the 1/2 decides wrongly (bias_predicate)

A searched seed (tools/find_small_uniforms.py) is a literal below.  Nothing trusts it: the crafting finds the step and u from the seed's
stream and the oracle's word count every time and asserts the tier.  The searched points of a row are its first crafted points, in step
order; each was searched under the row as it stands with the earlier ones placed, which the crafting reproduces."""
import math
from decimal import Decimal, localcontext

import numpy as np

import mcq_amd
from oracle import oracle
from tests.near_tie_util import Case, _Streams, _bits, _from_bits, _probe, accept_bit, signed_ulps, uniform_of  # noqa: F401

abi = mcq_amd.abi

N_SETS = 5
HIGH, LOW, RARE, NEG, SPECIAL = range(N_SETS)
SET_NAMES = ("high", "low", "rare", "negative", "special")
FIRST_STEP, GAP, WALK = 4, 2, 400
P27 = 134217728.0  # 2^27

# regions: bounds on x = -ln u; tiers: bounds [lo, hi) on a27 = floor(u 2^27)
X_TOP = (2.0 ** -12, 2.0 ** -9)
REGION_X = {"high": (2.0 ** -12, 0.05), "mid": (0.05, 1.0), "low-1": (1.0, 4.0), "low-2": (4.0, 9.0)}
TIERS = {"low-3": (300, 16000), "low-4": (4, 64), "low-5": (1, 4), "zero": (0, 1),
         "top": (int(math.ceil(math.exp(-X_TOP[1]) * P27)) + 1, int(math.exp(-X_TOP[0]) * P27))}
EDGE_DELTAS = tuple(s * m for m in (2.0 ** -30, 2.0 ** -16, 0.9 * 2.0 ** -10, 1.1 * 2.0 ** -10) for s in (1.0, -1.0))

# What each natural set is asked for, as (region, kind, spec).  A set places whichever of them some chain's step allows first, in this
# order: the rarer region in front.  spec: ("ulp", d), ("rel", delta) or ("relx", f) for delta = f x.
HIGH_PLAN = (tuple(("high", "count", ("ulp", d)) for d in (2, -2, 3, -3)) + tuple(("high", "miss", ("ulp", d)) for d in (8, -8)) +
             tuple(("high", "rel", ("relx", f)) for f in (-0.5, 0.125, -0.125, 2.0 ** -7, -2.0 ** -7)))  # the sixth, +x / 2, is the searched first point
LOW_PLAN = (tuple(("low-2", "rel", ("rel", d)) for d in EDGE_DELTAS + (2.0 ** -9, -2.0 ** -9)) + tuple(("low-1", "rel", ("rel", d)) for d in EDGE_DELTAS))
NEG_PLAN = (tuple(("low-2", "rel", ("rel", d)) for d in (1.1 * 2.0 ** -10, -1.1 * 2.0 ** -10)) +
            tuple(("mid", "count", ("ulp", d)) for d in (2, -2, 3, -3)) + tuple(("mid", "miss", ("ulp", d)) for d in (8, -8)) +
            tuple(("mid", "rel", ("rel", d)) for d in (2.0 ** -16, -2.0 ** -16, 1.1 * 2.0 ** -10, -1.1 * 2.0 ** -10)))
# The searched chains, as (tier, kind, spec): chain 0 of the high set, and chain i of the rare set for entry i, placed in this order
# unless the case has an entry in ORDER.
TOP_PLAN = (("top", "rel", ("relx", 0.5)),)
RARE_PLAN = (("zero", "abs", ("abs", 0.05)), ("zero", "abs", ("abs", -0.05)), ("low-5", "bias", ("abs", 0.05)), ("low-5", "bias", ("abs", -0.05)),
             ("low-4", "bias", ("abs", 0.05)), ("low-4", "bias", ("abs", -0.05)), ("low-4", "abs", ("abs", -3.0)),
             ("low-3", "rel", ("rel", 1.1 * 2.0 ** -10)), ("low-3", "rel", ("rel", -1.1 * 2.0 ** -10)), ("low-3", "abs", ("abs", 0.3)),
             ("low-3", "abs", ("abs", -0.3)))
PLANS = {HIGH: TOP_PLAN + HIGH_PLAN, LOW: LOW_PLAN, RARE: RARE_PLAN, NEG: NEG_PLAN}
PLANNED = sum(len(p) for p in PLANS.values())

SPECIAL_VALUES = (0.0, -0.0, float("nan"), float("inf"), float("-inf"), 5e-324, 1e-320, 1e-46, 1e-40, 1e39, 1e300, -1e300)
# What rule() must give per value and sign of dE, written out: (dE > 0, dE == 0, dE < 0), "a" accepts, "r" rejects (a u of exactly 0
# aside, which the crafting asserts no special step draws)
SPECIAL_EXPECTED = {"0.0": "aaa", "-0.0": "aaa", "nan": "aaa", "inf": "raa", "-inf": "aar", "5e-324": "aaa", "1e-320": "aaa", "1e-46": "aaa",
                    "1e-40": "aaa", "1e+39": "raa", "1e+300": "raa", "-1e+300": "aar"}
assert sorted(SPECIAL_EXPECTED) == sorted(repr(v) for v in SPECIAL_VALUES)


def rule(beta, dE, u):
    """The reference's accept decision u < min(1.0, exp(-beta dE)) in Python: min(1.0, nan) is 1.0, so a NaN accepts, and inf * 0 is one."""
    x = -beta * float(dE)
    e = float("inf") if x > 709.0 else math.exp(x)  # (math.exp raises where C's exp returns inf)
    return u < min(1.0, e)


def c32_of(beta):
    """The float32 the kernel's estimate works with: (float)(-beta log2(e))."""
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return float(np.float32(-beta * 1.4426950408889634))


class RangeCase(Case):
    """A case with an explicit seed array: consecutive seeds, with the literal seeds of the searched chains written over theirs."""

    def __init__(self, name, mode, N, lanes, n_steps, seed, trace=True, rng="mt19937", row=None):
        super().__init__(name, mode, N, lanes, n_sets=N_SETS, n_steps=n_steps, trace=trace, seed=seed, rng=rng)
        self.searched, self.row = SEARCHED[name], row  # a case without an entry fails here; None: still to be searched (the tool fills it)
        self.order = tuple(ORDER.get(name, range(len(RARE_PLAN))))
        assert sorted(self.order) == list(range(len(RARE_PLAN))) and (self.searched is None or len(self.searched) == len(TOP_PLAN) + len(RARE_PLAN))

    def rare_plan(self):
        """[(chain of the rare set, entry of RARE_PLAN)] in the order the case places them."""
        return [(i, RARE_PLAN[i]) for i in self.order]

    def seeds(self, searching=False):
        s = [self.seed + i for i in range(self.n_chains)]
        if self.searched is None and not searching:
            raise ValueError(f"{self.name}: no searched seeds yet: tools/find_small_uniforms.py {self.name}")
        if self.searched is not None:
            s[HIGH * self.set_chains] = self.searched[0]
            for i, v in enumerate(self.searched[1:]):
                s[RARE * self.set_chains + i] = v
        return np.array(s, dtype=np.uint32)

    def base_schedules(self):
        out = super().base_schedules()
        out[NEG] = {"type": "linear_annealing", "beta_start": -0.2, "beta_end": -0.9}
        return out


# tools/find_small_uniforms.py's output: per case the seed of the high set's first chain, then those of the rare set in RARE_PLAN's order
SEARCHED = {
    "board6_g2": (1000033, 14159822, 11008812, 14151382, 13512553, 11052375, 12373707, 10460816, 1000230, 1000275, 1000912, 1001032),
    "board12_g4": (2000007, 21543435, 22289514, 20809125, 20595619, 21582417, 21116601, 21611238, 2001672, 2001852, 2002204, 2002432),
    "board12_g8": (3000009, 32361290, 31658334, 32802579, 33192639, 32766657, 30073526, 32122947, 3000189, 3001099, 3001120, 3001235),
    "board17_g16": (4000016, 41486673, 46462140, 41856213, 43804884, 45007134, 46631558, 40873807, 4000262, 4000476, 4000579, 4000820),
    "board12_reduced": (5000023, 55995927, 55979427, 54366242, 51084290, 54585695, 51399812, 54968255, 5000506, 5000753, 5001469, 5001918),
    "full3d6_g8": (6000010, 62018630, 61226631, 61992535, 63029280, 62952375, 61030529, 60824787, 6000587, 6000787, 6000799, 6000855),
    "full3d10_g4": (7000007, 70552893, 72489165, 71491011, 72463159, 72092231, 71121635, 71192464, 7000140, 7000397, 7000621, 7001353),
    "full3d40": (8000012, 81233295, 81149828, 81403762, 81301697, 81164712, 80808488, 81170816, 8000058, 8000066, 8000364, 8000704),
    "p_board12_g4": (9000080, 95036972, 95332966, 90384943, 92369729, 94341334, 90393870, 95126879, 9000822, 9000899, 9001012, 9002379),
    "p_full3d9_g8": (10000005, 103691399, 100315239, 102943907, 101275506, 101562954, 102437296, 101534627, 10000481, 10001020, 10001385, 10001415),
}
# the order in which a case places the entries of RARE_PLAN where it is not the plan's own (the tool's output as well): the four rarest
# points of the wide case stand where its stream has them, and the placing follows their steps
ORDER = {
    "full3d40": (3, 5, 4, 6, 2, 0, 1, 7, 8, 9, 10),
}
# name, mode, N, lanes, steps, first seed, ..., and the row of SWEEP_TABLE the launch must select, as
# (MODE, G, PATIENCE, NT, REDUCED, PHILOX, NC, EXCH, CAND5, EARLYU, SLIM, CNT, WIDE)
CASES = (
    RangeCase("board6_g2", "board", 6, 2, 450, 31000, row=(0, 2, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0)),
    RangeCase("board12_g4", "board", 12, 4, 430, 32000, row=(0, 4, 0, 3, 0, 0, 12, 0, 0, 0, 0, 0, 0)),
    RangeCase("board12_g8", "board", 12, 8, 451, 33000, row=(0, 8, 0, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0)),
    RangeCase("board17_g16", "board", 17, 16, 470, 34000, row=(0, 16, 0, 2, 0, 0, 0, 0, 0, 1, 0, 0, 0)),
    RangeCase("board12_reduced", "board", 12, 0, 445, 35000, trace="reduced", row=(0, 16, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0)),
    RangeCase("full3d6_g8", "full_3d", 6, 8, 421, 36000, row=(1, 8, 0, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0)),
    RangeCase("full3d10_g4", "full_3d", 10, 4, 438, 37000, row=(1, 4, 0, 5, 0, 0, 0, 0, 0, 0, 1, 0, 0)),
    RangeCase("full3d40", "full_3d", 40, 0, 300, 38000, row=(1, 16, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1)),
    RangeCase("p_board12_g4", "board", 12, 4, 430, 39000, rng="philox", row=(0, 4, 0, 3, 0, 1, 12, 0, 0, 0, 0, 0, 0)),
    RangeCase("p_full3d9_g8", "full_3d", 9, 8, 429, 40000, rng="philox", row=(1, 8, 0, 3, 0, 1, 0, 0, 0, 0, 0, 0, 0)),
)
CASES_BY_NAME = {c.name: c for c in CASES}


# ---- beta for a wanted place of the probability ---------------------------------------------------------------------------------------

def _beta_rel(delta, dE, u):
    target = u * (1.0 + delta)
    if not 0.0 < target < 1.0:
        return None
    beta = -math.log(target) / dE
    prob = math.exp(-beta * dE)
    ok = 0.0 < prob < 1.0 and abs((prob - u) / u - delta) <= 0.01 * abs(delta) and abs(signed_ulps(prob, u)) > 1000
    return beta if ok else None


def _beta_abs(eta, dE, u):
    target = u + eta / P27
    if not 0.0 < target < 1.0:
        return None
    beta = -math.log(target) / dE
    prob = math.exp(-beta * dE)
    ok = 0.0 < prob < 1.0 and abs((prob - u) * P27 - eta) <= 0.01 * abs(eta) and abs(signed_ulps(prob, u)) > 1000
    return beta if ok else None


def _beta_ulp(d, dE, u):
    """As near_tie_util._beta_for, but the walk starts at the beta of the wanted value, not of u: at a small x one ulp of the
    probability is many ulp of beta."""
    target = _from_bits(_bits(u) + d)
    if not 0.0 < target < 1.0:
        return None
    b0 = _bits(-math.log(target) / dE)
    for k in range(2 * WALK + 1):
        beta = _from_bits(b0 + ((k + 1) // 2 if k & 1 else -(k // 2)))
        prob = math.exp(-beta * dE)
        if 0.0 < prob < 1.0 and signed_ulps(prob, u) == d:
            return beta
    return None


def bias_predicate(u, prob):
    """True where float32 arithmetic without the 1/2 in w decides wrongly: a27 + 1/2 against p27 = prob 2^27 lies outside a bracket of
    p27 2^-10 alone, on the wrong side."""
    a, p27 = math.floor(u * P27), prob * P27
    return abs(a + 0.5 - p27) > p27 * 2.0 ** -10 and ((a + 0.5 < p27) != (u < prob))


def _beta_for(kind, spec, dE, u):
    if dE == 0 or not 0.0 < u < 1.0:
        return None
    x = -math.log(u)
    if spec[0] == "ulp":
        return _beta_ulp(spec[1], dE, u) if x <= 1.0 else None
    if spec[0] != "abs":
        return _beta_rel(spec[1] * x if spec[0] == "relx" else spec[1], dE, u)
    beta = _beta_abs(spec[1], dE, u)
    if beta is not None and kind == "bias":
        # eta = +0.05 where the fraction of u 2^27 is below 0.4, -0.05 where it is above 0.6; and clear of the edge of the wrong
        # kernel's own bracket by that bracket again plus 0.02, so that its float32 rounding cannot save it
        a, f, prob = math.floor(u * P27), u * P27 - math.floor(u * P27), math.exp(-beta * dE)
        if not ((f < 0.4) if spec[1] > 0 else (f > 0.6)) or not bias_predicate(u, prob) or abs(a + 0.5 - prob * P27) <= prob * P27 * 2.0 ** -9 + 0.02:
            return None
    return beta


def _in_region(region, x):
    lo, hi = REGION_X[region]
    return lo <= x < hi if region == "high" else lo <= x <= hi if region == "mid" else lo < x <= hi


# ---- probes ---------------------------------------------------------------------------------------------------------------------------

def _params(case, tab, n_chains):
    p = abi.make_params(case.N, tab.shape[1], "random", case.base_schedules()[0], n_chains, mcmc_type=case.mode, Q=case.Q, rng=case.rng)
    p._schedules, p.beta_table, p._beta_keepalive = None, tab.ctypes.data, tab
    return p


def _probe_set(case, streams, seeds_t, row, s):
    """near_tie_util._probe for all chains of a set in one oracle run: [(dE, u)] of step s under row[:s] and beta(s) = 0."""
    tab = np.ascontiguousarray(row[: s + 1]).reshape(1, s + 1).copy()
    tab[0, s] = 0.0
    res = oracle.run(_params(case, tab, len(seeds_t)), seeds_t, states=False, words=True, n_threads=8)
    assert (res["hist_len"] == s + 2).all()
    h = res["energy_hist"]
    return [(int(h[r, s + 1]) - int(h[r, s]), uniform_of(*streams.pair_before(int(seeds_t[r]), int(res["rng_words"][r])))) for r in range(len(seeds_t))]


def words_after(case, seed, row, k):
    """The words chain `seed` has drawn after k steps under row[:k] (the uniform of step k - 1 is the last two of them)."""
    tab = np.ascontiguousarray(row[:k]).reshape(1, k).copy()
    return int(oracle.run(_params(case, tab, 1), np.array([seed], dtype=np.uint32), trace=False, states=False, words=True)["rng_words"][0])


def step_of_word(case, seed, row, j, known=None):
    """The step whose uniform starts at word j of the chain's stream, by bisection on the oracle's word count; None if there is none in
    front of the last step.  `known`: counts already asked for under this row, by number of steps."""
    known = {} if known is None else known

    def count(k):
        if k not in known:
            known[k] = words_after(case, seed, row, k)
        return known[k]

    lo, hi = 1, case.n_steps - 1
    if count(hi) < j + 2:
        return None
    while lo < hi:
        mid = (lo + hi) // 2
        if count(mid) >= j + 2:
            hi = mid
        else:
            lo = mid + 1
    return lo - 1 if count(lo) == j + 2 else None


def small_uniform_step(case, streams, seed, row, tier, kind, spec, after):
    """(step, dE, u, beta) of the first place of the seed's stream whose first word puts a27 into the tier and that is the uniform of a step
    >= `after` with dE > 0 at which the wanted point can stand; None if the chain has none."""
    lo, hi = TIERS[tier]
    known = {}
    total = known[case.n_steps - 1] = words_after(case, seed, row, case.n_steps - 1)
    streams.pair_before(seed, total)
    a = streams.words[seed][:total].astype(np.int64) >> 5
    for j in np.nonzero((a >= lo) & (a < hi))[0]:
        s = step_of_word(case, seed, row, int(j), known) if j + 2 <= total else None
        if s is None or s < after:
            continue
        dE, u = _probe(case, streams, seed, row, s, None)
        assert math.floor(u * P27) == a[j], "the word count names another pair"
        beta = _beta_for(kind, spec, dE, u) if dE > 0 else None
        if beta is not None:
            return s, dE, u, beta
    return None


# ---- crafting -------------------------------------------------------------------------------------------------------------------------

def _point(t, c, s, dE, u, beta, kind, region, spec):
    prob = math.exp(-beta * dE)
    return {"set": t, "chain": int(c), "step": int(s), "dE": int(dE), "u": u, "beta": beta, "prob": prob, "accept": bool(u < prob), "kind": kind,
            "ulps": signed_ulps(prob, u), "counts": 1 if kind == "count" else 0, "region": region, "spec": spec, "x": -math.log(u),
            "a27": math.floor(u * P27)}


def _place_searched(case, table, seeds, streams, points, t, i, entry, after, search):
    tier, kind, spec = entry
    c = t * case.set_chains + i
    if search is not None:
        seeds[c] = search(case, streams, table[t], entry, after)
    found = small_uniform_step(case, streams, int(seeds[c]), table[t], tier, kind, spec, after)
    assert found is not None, f"{case.name}: seed {int(seeds[c])} holds no {tier} {kind} point behind step {after}"
    s, dE, u, beta = found
    table[t, s] = beta
    points.append(_point(t, c, s, dE, u, beta, kind, tier, spec))
    return s + 1 + GAP


def _place_natural(case, table, seeds, streams, points, t, plan, s, negative=False):
    n, row, wanted = case.set_chains, table[t], list(plan)
    seeds_t = np.ascontiguousarray(seeds[t * n: (t + 1) * n])
    while wanted and s < case.n_steps - 1:
        probes, hit = _probe_set(case, streams, seeds_t, row, s), None
        for w in wanted:
            for k in range(n):
                r = (k + 5 * len(points)) % n  # spread the points over the set's chains
                dE, u = probes[r]
                if (dE < 0 if negative else dE > 0) and 0.0 < u < 1.0 and _in_region(w[0], -math.log(u)):
                    beta = _beta_for(w[1], w[2], dE, u)
                    if beta is not None:
                        hit = (w, r, dE, u, beta)
                        break
            if hit:
                break
        if hit is None:
            s += 1
            continue
        w, r, dE, u, beta = hit
        row[s] = beta
        points.append(_point(t, t * n + r, s, dE, u, beta, w[1], w[0], w[2]))
        wanted.remove(w)
        s += 1 + GAP


def _with_zero_dE_first(v):
    return math.isinf(v) or math.isnan(v)  # inf * 0 is what a dE of 0 is there for


def _place_special(case, table, seeds, streams, points, t, s):
    """The twelve values at twelve steps at which three chains or more have dE > 0 and three or more dE < 0 (the beta = 0 probe); the
    infinities and NaN take the steps at which a chain has dE = 0 as long as there are such.  One point per chain and step."""
    n, row, pending = case.set_chains, table[t], list(SPECIAL_VALUES)
    seeds_t = np.ascontiguousarray(seeds[t * n: (t + 1) * n])
    while pending and s < case.n_steps - 1:
        probes = _probe_set(case, streams, seeds_t, row, s)
        dEs = [dE for dE, _ in probes]
        if sum(d > 0 for d in dEs) < 3 or sum(d < 0 for d in dEs) < 3 or not all(0.0 < u < 1.0 for _, u in probes):
            s += 1
            continue
        first = [i for i, v in enumerate(pending) if _with_zero_dE_first(v) == (0 in dEs)]
        beta = pending.pop(first[0] if first else 0)
        row[s] = beta
        for r, (dE, u) in enumerate(probes):
            points.append({"set": t, "chain": t * n + r, "step": int(s), "dE": int(dE), "u": u, "beta": beta, "prob": None, "accept": bool(rule(beta, dE, u)),
                           "kind": "special", "ulps": 0, "counts": 0, "region": "special", "spec": ("beta", repr(beta)), "x": -math.log(u),
                           "a27": math.floor(u * P27)})
        s += 1 + GAP


def craft(case, search=None):
    """(table [5][n_steps], points, seeds).  One dict per crafted point as in near_tie_util.craft, plus region (or tier), spec, x = -ln u and
    a27; a special step gives one point per chain of its set (kind "special", accept from rule()).  `search`
    (tools/find_small_uniforms.py): a function that looks for the seed of a searched chain; without it the case's literals are used."""
    table, seeds, streams, points = case.base_table(), case.seeds(searching=search is not None).copy(), _Streams(case.rng), []
    s = _place_searched(case, table, seeds, streams, points, HIGH, 0, TOP_PLAN[0], FIRST_STEP, search)
    _place_natural(case, table, seeds, streams, points, HIGH, HIGH_PLAN, s)
    _place_natural(case, table, seeds, streams, points, LOW, LOW_PLAN, FIRST_STEP)
    s = FIRST_STEP
    for i, entry in case.rare_plan():
        s = _place_searched(case, table, seeds, streams, points, RARE, i, entry, s, search)
    _place_natural(case, table, seeds, streams, points, NEG, NEG_PLAN, FIRST_STEP, negative=True)
    _place_special(case, table, seeds, streams, points, SPECIAL, FIRST_STEP)
    return table, points, seeds


_crafted = {}


def crafted(name):
    """craft() of a listed case, once per process: (table, points), shared and left unchanged."""
    if name not in _crafted:
        case = CASES_BY_NAME[name]
        table, points, seeds = craft(case)
        assert (seeds == case.seeds()).all()
        table.setflags(write=False)
        _crafted[name] = (table, tuple(points))
    return _crafted[name]


def expected_near_ties(case, points):
    want = np.zeros(case.n_chains, dtype=np.int64)
    for pt in points:
        want[pt["chain"]] += pt["counts"]
    return want


def crafted_points(points):
    return [pt for pt in points if pt["kind"] != "special"]


def special_steps(points):
    """{step: its points, one per chain of the set}"""
    out = {}
    for pt in points:
        if pt["kind"] == "special":
            out.setdefault(pt["step"], []).append(pt)
    return out


# ---- the checks -----------------------------------------------------------------------------------------------------------------------

def check_against_decimal(pt):
    """exp at 60 digits from the exact decimal values of the float64 beta, dE and u.  Every implementation -- the reference, the oracle, the
    kernel -- rounds the product x = -beta dE to float64 before exp sees it, which alone moves exp(x) by up to |x| ulp.  So glibc's
    exp is held to 1 ulp of the decimal exp of that float64 x, with the decimal's side of u; and the decimal exp of the unrounded
    product lies within 1 + |x| ulp of glibc's result, on the same side of u at every point that is no tie.  Returns glibc's error in ulp
    against the one and against the other."""
    with localcontext() as ctx:
        ctx.prec = 60
        x = -pt["beta"] * float(pt["dE"])
        dec, unrounded = Decimal(x).exp(), (-(Decimal(pt["beta"]) * pt["dE"])).exp()
        prob, u, ulp = Decimal(pt["prob"]), Decimal(pt["u"]), Decimal(math.ulp(pt["prob"]))
        assert pt["prob"] == math.exp(x) and abs(prob - dec) <= ulp, (pt, dec)
        assert dec != u and (prob > u) == (dec > u) and (prob > u) == pt["accept"], (pt, dec)
        assert abs(prob - unrounded) <= (1 + Decimal(abs(x))) * ulp, (pt, unrounded)
        assert pt["kind"] in ("count", "miss") or (unrounded > u) == pt["accept"], (pt, unrounded)
        return float((prob - dec) / ulp), float((prob - unrounded) / ulp)


def _specs(pts):
    return sorted((pt["region"], pt["kind"], pt["spec"]) for pt in pts)


def check_plan_was_met(case, points):
    """Every minimum the plan sets, per case, and that no planned point was skipped: a crafting that places less fails here and not as a
    weaker test."""
    name, n = case.name, case.set_chains
    assert case.n_sets >= 5 and 300 <= case.n_steps <= 470 and 80 <= case.n_chains <= 192 and n == (32 if case.lanes == 2 else 16)
    real, special = crafted_points(points), special_steps(points)
    assert len(real) == PLANNED, f"{name}: {len(real)} points of {PLANNED} planned"
    for t, plan in PLANS.items():
        got = _specs(pt for pt in real if pt["set"] == t)
        assert got == sorted(plan), f"{name}: set {SET_NAMES[t]}: planned and not placed: {sorted(set(plan) - set(got))}"
    seen = set()
    for pt in points:
        assert (pt["chain"], pt["step"]) not in seen and pt["chain"] // n == pt["set"] and FIRST_STEP <= pt["step"] < case.n_steps - 1
        seen.add((pt["chain"], pt["step"]))
    for pt in real:
        assert 0.0 < pt["u"] < 1.0 and 0.0 < pt["prob"] < 1.0 and pt["accept"] == (pt["ulps"] > 0) and pt["beta"] * pt["dE"] > 0, pt
        assert abs(pt["ulps"]) == abs(pt["spec"][1]) if pt["kind"] in ("count", "miss") else abs(pt["ulps"]) > 1000, pt
        assert pt["kind"] not in ("count", "miss") or pt["x"] <= 1.0, pt
        assert (pt["dE"] < 0 and pt["beta"] < 0) if pt["set"] == NEG else (pt["dE"] > 0 and pt["beta"] > 0), pt
        if pt["region"] in REGION_X:
            assert _in_region(pt["region"], pt["x"]), pt
        else:
            assert TIERS[pt["region"]][0] <= pt["a27"] < TIERS[pt["region"]][1], pt
        check_against_decimal(pt)
    by = lambda t, region, kind: [pt for pt in real if pt["set"] == t and pt["region"] == region and pt["kind"] == kind]  # noqa: E731
    rel = lambda pt: (pt["prob"] - pt["u"]) / pt["u"]  # noqa: E731
    eta = lambda pt: (pt["prob"] - pt["u"]) * P27  # noqa: E731
    near = lambda got, want: len(got) == len(want) and all(abs(g - w) <= 0.02 * abs(w) for g, w in zip(sorted(got), sorted(want)))  # noqa: E731
    # high: probabilities next to 1
    assert sorted(pt["ulps"] for pt in by(HIGH, "high", "count")) == [-3, -2, 2, 3] and sorted(pt["ulps"] for pt in by(HIGH, "high", "miss")) == [-8, 8]
    high_rel = by(HIGH, "high", "rel") + by(HIGH, "top", "rel")
    assert len(high_rel) >= 6 and all(abs(rel(pt)) <= 0.51 * pt["x"] for pt in high_rel) and {rel(pt) > 0 for pt in high_rel} == {True, False}
    assert any(X_TOP[0] <= pt["x"] < X_TOP[1] for pt in real if pt["set"] == HIGH), f"{name}: no point with x < 2^-9"
    assert all(REGION_X["high"][0] <= pt["x"] < REGION_X["high"][1] for pt in real if pt["set"] == HIGH)
    # low-1, low-2: natural
    assert near([rel(pt) for pt in by(LOW, "low-1", "rel")], EDGE_DELTAS), name
    assert near([rel(pt) for pt in by(LOW, "low-2", "rel")], EDGE_DELTAS + (2.0 ** -9, -2.0 ** -9)), name
    # low-3 .. zero: searched, each the first points of the rare row in step order
    assert near([rel(pt) for pt in by(RARE, "low-3", "rel")], (1.1 * 2.0 ** -10, -1.1 * 2.0 ** -10)) and near([eta(pt) for pt in by(RARE, "low-3", "abs")], (0.3, -0.3))
    assert near([eta(pt) for pt in by(RARE, "low-4", "abs")], (-3.0,))
    for tier in ("low-4", "low-5"):
        bias = by(RARE, tier, "bias")
        assert sorted(pt["accept"] for pt in bias) == [False, True], (name, tier)
        for pt in bias:
            f = pt["u"] * P27 - pt["a27"]
            assert bias_predicate(pt["u"], pt["prob"]) and (f < 0.4 and eta(pt) > 0 if pt["accept"] else f > 0.6 and eta(pt) < 0) and abs(abs(eta(pt)) - 0.05) < 0.001, pt
    zero = by(RARE, "zero", "abs")
    assert near([eta(pt) for pt in zero], (0.05, -0.05)) and all(pt["a27"] == 0 and 0.0 < pt["prob"] * P27 < 1.0 and pt["x"] > 18.7 for pt in zero), name
    rare_steps = [pt["step"] for pt in real if pt["set"] == RARE]
    assert rare_steps == sorted(rare_steps) and [pt["chain"] for pt in real if pt["set"] == RARE] == [RARE * n + i for i, _ in case.rare_plan()]
    assert [pt for pt in real if pt["set"] == HIGH][0]["chain"] == HIGH * n and [pt for pt in real if pt["set"] == HIGH][0]["region"] == "top"
    # negative beta
    assert (case.base_table()[NEG] < 0).all()
    assert sorted(pt["ulps"] for pt in by(NEG, "mid", "count")) == [-3, -2, 2, 3] and sorted(pt["ulps"] for pt in by(NEG, "mid", "miss")) == [-8, 8]
    assert near([rel(pt) for pt in by(NEG, "mid", "rel")], (2.0 ** -16, -2.0 ** -16, 1.1 * 2.0 ** -10, -1.1 * 2.0 ** -10))
    assert near([rel(pt) for pt in by(NEG, "low-2", "rel")], (1.1 * 2.0 ** -10, -1.1 * 2.0 ** -10))
    # special values
    assert len(special) == len(SPECIAL_VALUES), f"{name}: {len(special)} special steps"
    assert sorted(_bits(pts[0]["beta"]) for pts in special.values()) == sorted(_bits(v) for v in SPECIAL_VALUES)
    steps = sorted(special)
    assert all(b - a > GAP for a, b in zip(steps, steps[1:]))
    zeros = 0
    for pts in special.values():
        assert len(pts) == n and {pt["set"] for pt in pts} == {SPECIAL} and len({_bits(pt["beta"]) for pt in pts}) == 1
        assert sum(pt["dE"] > 0 for pt in pts) >= 3 and sum(pt["dE"] < 0 for pt in pts) >= 3, (name, pts[0]["step"])
        zeros += sum(pt["dE"] == 0 for pt in pts)
        for pt in pts:
            want = SPECIAL_EXPECTED[repr(pt["beta"])][0 if pt["dE"] > 0 else 1 if pt["dE"] == 0 else 2]
            assert 0.0 < pt["u"] < 1.0 and pt["accept"] == (want == "a") == bool(rule(pt["beta"], pt["dE"], pt["u"])), pt
    assert zeros >= 1, f"{name}: no special step with dE = 0"
    c32 = {repr(v): c32_of(v) for v in SPECIAL_VALUES}
    assert c32["1e-46"] == 0.0 and 0.0 < abs(c32["1e-40"]) < 1.1754943508222875e-38 and math.isinf(c32["1e+39"]) and math.isnan(c32["nan"])


def describe(pt):
    return f"{SET_NAMES[pt['set']]} set, {pt['region']} {pt['kind']} {pt['spec']}, a27 {pt['a27']}, x {pt['x']:.6g}"
