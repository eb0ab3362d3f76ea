"""CPU only: the crafted cases of tests/accept_range_util.py -- probabilities next to 1, probabilities below 2^-13 down to the last 2^-27
cell, negative beta and special beta values.  The plan of every case is met; the oracle, naive and fast, counts exactly the crafted ties and
decides every crafted and every special point as the util's Python truth says; the truth agrees with decimal arithmetic at 60 digits; the
searched seeds hold what they were searched for; every case selects its row of SWEEP_TABLE; and near_tie_util's own tables are what they were."""
import math

import numpy as np
import pytest

import mcq_amd
from oracle import oracle
from tests import accept_range_util as ar
from tests import near_tie_util as nt
from tests import variant_cases as vc
from tests.test_philox_ties_host import BEFORE, _digest

abi = mcq_amd.abi
NAMES = [c.name for c in ar.CASES]
F = abi.SWEEP_VARIANT_FIELDS


@pytest.mark.parametrize("name", NAMES)
def test_plan_was_met(name):
    """Every minimum of the plan, no planned point skipped, the bias predicate and the decimal cross-check at every point."""
    case = ar.CASES_BY_NAME[name]
    table, points = ar.crafted(name)
    ar.check_plan_was_met(case, points)
    assert np.isnan(table[ar.SPECIAL]).sum() == 1 and np.isinf(table[ar.SPECIAL]).sum() == 2 and np.isfinite(np.delete(table, ar.SPECIAL, axis=0)).all()
    errors = [ar.check_against_decimal(pt) for pt in ar.crafted_points(points)]
    assert max(abs(e) for e, _ in errors) <= 1.0 and all(abs(f) <= 1.0 + pt["x"] for (_, f), pt in zip(errors, ar.crafted_points(points)))


@pytest.mark.parametrize("name", NAMES)
def test_oracle_counts_the_crafted_ties_and_decides_as_python(name):
    case = ar.CASES_BY_NAME[name]
    table, points = ar.crafted(name)
    seeds, want = case.seeds(), ar.expected_near_ties(case, points)
    assert int(want.sum()) == 8 and int(want.max()) >= 1
    runs = {"oracle": oracle.run(case.params(table, trace=True), seeds, n_threads=4),
            "fast oracle": oracle.run(case.params(table, trace=True), seeds, n_threads=4, fast=True)}
    for what, res in runs.items():
        np.testing.assert_array_equal(res["near_ties"], want, err_msg=f"{name}: {what}: near_ties per chain")
        assert (res["hist_len"] == case.n_steps + 1).all()
        for pt in points:
            c, s = pt["chain"], pt["step"]
            assert nt._bits(float(table[pt["set"], s])) == nt._bits(pt["beta"])
            if pt["kind"] != "special":
                assert pt["accept"] == (pt["u"] < math.exp(-pt["beta"] * pt["dE"]))
            assert pt["accept"] == bool(ar.rule(pt["beta"], pt["dE"], pt["u"]))
            assert nt.accept_bit(res, c, s) == int(pt["accept"]), f"{name}: {what}: chain {c} step {s}: {ar.describe(pt)}, beta {pt['beta']!r}, dE {pt['dE']}, u {pt['u']!r}"
            assert int(res["energy_hist"][c, s + 1]) - int(res["energy_hist"][c, s]) == (pt["dE"] if pt["accept"] else 0), (name, what, c, s)
    for k in runs["oracle"]:
        np.testing.assert_array_equal(runs["oracle"][k], runs["fast oracle"][k], err_msg=f"{name}: fast oracle vs oracle: {k}")
    control = oracle.run(case.params(case.base_table()), seeds, trace=case.trace, n_threads=4, fast=True)
    assert int(control["near_ties"].sum()) == 0, f"{name}: the uncrafted table ties by itself"
    # the chains of the negative row move both ways under it: its uncrafted steps are decisions too
    neg = slice(ar.NEG * case.set_chains, (ar.NEG + 1) * case.set_chains)
    moves = np.diff(runs["oracle"]["energy_hist"][neg, : case.n_steps + 1].astype(np.int64), axis=1)
    assert (moves > 0).sum() > 100 and (moves < 0).sum() > 100


@pytest.mark.parametrize("name", NAMES)
def test_searched_literals_hold_their_tiers(name):
    """The uniform of every searched point, looked up again from the seed alone: the chain's word count after the point's step under the
    crafted row names two words of the stream -- NumPy's own MT19937 on that stream -- and they put a27 into the tier."""
    case = ar.CASES_BY_NAME[name]
    table, points = ar.crafted(name)
    searched = [pt for pt in ar.crafted_points(points) if pt["region"] in ar.TIERS]
    assert len(searched) == len(case.searched) == 12 and len(set(case.searched)) == 12 and all(s > 0 for s in case.searched)
    n = case.set_chains
    assert {pt["chain"]: int(case.seeds()[pt["chain"]]) for pt in searched} == dict(zip([ar.HIGH * n] + [ar.RARE * n + i for i in range(11)], case.searched))
    for pt in searched:
        seed = int(case.seeds()[pt["chain"]])
        words = ar.words_after(case, seed, table[pt["set"]], pt["step"] + 1)
        if case.rng == "mt19937":
            rs = np.random.RandomState(seed)
            rs.randint(0, 2**32, size=words - 2, dtype=np.uint32)
            u = rs.random_sample()
        else:
            w = oracle.rng_stream(seed, "u32", words, rng="philox")
            u = nt.uniform_of(w[-2], w[-1])
        lo, hi = ar.TIERS[pt["region"]]
        assert u == pt["u"] and lo <= math.floor(u * ar.P27) < hi and pt["dE"] > 0, (name, pt)


def test_cases_select_their_rows():
    """The ten launches the plan lists, each on its row of SWEEP_TABLE, with the sizes, lanes and traces of near_tie_util's cases of these names."""
    assert NAMES == ["board6_g2", "board12_g4", "board12_g8", "board17_g16", "board12_reduced", "full3d6_g8", "full3d10_g4", "full3d40", "p_board12_g4",
                     "p_full3d9_g8"]
    reachable = set(vc.reachable_rows())
    for case in ar.CASES:
        v = mcq_amd._lib.sweep_variant(case.params(case.base_table()))
        row = tuple(int(v[k]) for k in F)
        assert row == case.row and row in reachable, (case.name, dict(zip(F, row)))
        assert v["SLIM"] == (case.name == "full3d10_g4") and v["WIDE"] == (case.name == "full3d40") and (not case.lanes or v["G"] == case.lanes)
        assert v["PHILOX"] == (case.rng == "philox") and v["REDUCED"] == (case.trace == "reduced") and not v["EXCH"] and not v["PATIENCE"]
        old = nt.CASES_BY_NAME["p_board17_g16" if case.name == "board17_g16" else case.name]
        assert (old.mode, old.N, old.lanes, old.trace, old.Q) == (case.mode, case.N, case.lanes, case.trace, case.Q)
        assert old.rng == case.rng or case.name == "board17_g16"
        if case.rng == "philox":
            assert tuple(int(v[k]) for k in ("MODE", "G", "PATIENCE", "NT", "REDUCED", "NC")) == nt.PHILOX_ROW[case.name]
    assert len({c.row for c in ar.CASES}) == len(ar.CASES) == 10
    seeds = np.concatenate([c.seeds() for c in ar.CASES])
    assert len(set(seeds.tolist())) == len(seeds), "every chain of every case its own seed"
    old_seeds = {int(s) for c in nt.CASES + nt.PHILOX_CASES for s in c.seeds()}
    assert not old_seeds & set(seeds.tolist())


def test_special_rule_is_the_written_table():
    """rule() on every special value and sign of dE gives what SPECIAL_EXPECTED writes out, and min(1.0, nan) semantics are Python's."""
    assert min(1.0, float("nan")) == 1.0 and math.isnan(float("inf") * 0.0)
    for v in ar.SPECIAL_VALUES:
        got = "".join("a" if ar.rule(v, dE, 0.37) else "r" for dE in (3, 0, -3))
        assert got == ar.SPECIAL_EXPECTED[repr(v)], (v, got)
    assert ar.rule(float("inf"), 2, 0.0) is False and ar.rule(1.0, 2, 0.1) and not ar.rule(1.0, 2, 0.2)


@pytest.mark.parametrize("name", ("board12_g4", "board12_patience"))
def test_near_tie_tables_are_unchanged(name):
    """Importing this module's util leaves near_tie_util's bounds, cases and crafted tables bit-identical."""
    assert (nt.X_MIN, nt.X_MAX, nt.WALK) == (0.05, 1.0, 400) and len(nt.CASES) == 14 and len(nt.PHILOX_CASES) == 26
    assert not any(isinstance(c, ar.RangeCase) for c in nt.CASES_BY_NAME.values())
    table, points = nt.crafted(name)
    assert _digest(table, points) == BEFORE[name][0] and len(points) == BEFORE[name][1]
