"""CPU only: the oracle's swap decision, its tie count on the lower chain, and its accept decision at beta(step) * ladder[rung], on beta
tables crafted to put the uniform next to the probability under replica exchange (tests/exchange_tie_util.py).  The oracle is what the
kernels are compared with (tests/test_exchange_ties.py), so it is pinned here against the crafted counts and against each decision
recomputed in Python from (u, beta, the energies, the ladder)."""
import numpy as np
import pytest

import mcq_amd
from oracle import oracle
from tests import exchange_tie_util as xt
from tests import near_tie_util as nt

abi = mcq_amd.abi
NAMES = [c.name for c in xt.CASES]


def test_the_cases_run_every_exchange_kernel_of_the_mt19937_stream():
    """Together the cases run all nine rows of SWEEP_TABLE with EXCH and without PHILOX, each at the lane count it names."""
    rows = set()
    for case in xt.CASES:
        v = mcq_amd._lib.sweep_variant(case.params(case.base_table()))
        assert v["EXCH"] and not v["PHILOX"] and not (v["PATIENCE"] or v["REDUCED"] or v["CAND5"] or v["EARLYU"] or v["SLIM"] or v["CNT"] or v["WIDE"]), (case.name, v)
        assert not case.lanes or v["G"] == case.lanes, (case.name, v)
        rows.add((v["MODE"], v["G"], v["NT"], v["NC"]))
    assert rows == xt.EXCHANGE_ROWS, sorted(xt.EXCHANGE_ROWS - rows)


def oracle_counts_the_crafted_ties_and_swaps_as_recomputed(name):
    """(tests/test_philox_ties_host.py runs the same on the Philox cases.)"""
    case = xt.CASES_BY_NAME[name]
    table, points = xt.crafted(name)
    xt.check_plan_was_met(case, points)
    seeds, want = case.seeds(), nt.expected_near_ties(case, points)
    for pt in xt.swap_points(points):
        assert want[pt["chain"]] >= pt["counts"] and pt["partner"] != pt["chain"]
    for fast, what in ((False, "oracle"), (True, "fast oracle")):
        res = oracle.run(case.params(table, trace=True), seeds, n_threads=4, fast=fast)
        np.testing.assert_array_equal(res["near_ties"], want, err_msg=f"{name}: {what}: near_ties per chain (a swap tie goes to the lower chain alone)")
        for pt in points:
            assert table[pt["set"], pt["step"]] == pt["beta"]
        for pt in xt.step_points(points):
            c, s = pt["chain"], pt["step"]
            acc = xt.recomputed(case, pt)
            assert acc == pt["accept"] and nt.accept_bit(res, c, s) == int(acc), f"{name}: {what}: chain {c} step {s} ({pt['kind']}, {pt['ulps']:+d} ulp): accept bit"
            assert int(res["energy_hist"][c, s + 1]) - int(res["energy_hist"][c, s]) == (pt["dE"] if acc else 0), (name, what, c, s)
        for t in range(case.n_sets):  # the decision of a swap point: a's rung after s + 1 steps of its set
            sub, lo = case.one_set(t), t * case.set_chains
            for pt in xt.swap_points(points):
                if pt["set"] != t:
                    continue
                a, b, s = pt["chain"] - lo, pt["partner"] - lo, pt["step"]
                runs = [oracle.run(sub.params(table[t: t + 1, :n], n_steps=n), sub.seeds(), states=False, fast=fast) for n in (s, s + 1)]
                assert int(runs[0]["exchange_rung"][a]) == pt["t"] and int(runs[0]["exchange_rung"][b]) == pt["t"] + 1, (name, what, pt)
                assert int(runs[1]["final_energy"][a]) - int(runs[1]["final_energy"][b]) == pt["dEab"], (name, what, pt)
                swap = xt.recomputed(case, pt)
                assert swap == pt["swap"] and (int(runs[1]["exchange_rung"][a]) == pt["t"] + 1) == swap, f"{name}: {what}: swap after step {s} of chains {pt['chain']}, {pt['partner']} ({pt['kind']}, {pt['ulps']:+d} ulp)"
                assert int(runs[1]["exchange_rung"][b]) == (pt["t"] if swap else pt["t"] + 1)
                assert int(runs[1]["n_exchanges"][a]) - int(runs[0]["n_exchanges"][a]) == int(swap)
                for c in (pt["chain"], pt["partner"]):  # the tie is a's, never b's
                    assert int(runs[1]["near_ties"][c - lo]) == sum(q["counts"] for q in points if q["chain"] == c and q["step"] <= s), (name, what, pt)
    if case.trace is not True:  # the counter does not depend on what is traced
        np.testing.assert_array_equal(oracle.run(case.params(table), seeds, trace=case.trace, n_threads=4)["near_ties"], want)
    control = oracle.run(case.params(case.base_table()), seeds, trace=case.trace, n_threads=4, fast=True)
    assert int(control["near_ties"].sum()) == 0 and int(control["n_exchanges"].sum()) > 0, f"{name}: the uncrafted table ties by itself"
    ones = oracle.run(case.params(table, ladder=np.ones(case.R)), seeds, trace=case.trace, n_threads=4, fast=True)
    assert int(ones["near_ties"].sum()) == 0, f"{name}: a ladder of ones has exp(x) = 1 at every event: no swap can tie"


@pytest.mark.parametrize("name", NAMES)
def test_oracle_counts_the_crafted_ties_and_swaps_as_recomputed(name):
    oracle_counts_the_crafted_ties_and_swaps_as_recomputed(name)


def test_crafted_swap_uniforms_are_the_streams_words():
    """The u of a crafted swap point is NumPy's own random_sample at that place of the lower chain's stream."""
    case = xt.CASES_BY_NAME["x_board6_g4"]
    table, points = xt.crafted(case.name)
    pt = xt.swap_points(points)[0]
    sub, a = case.one_set(pt["set"]), pt["chain"] - pt["set"] * case.set_chains
    n = pt["step"] + 1
    words = int(oracle.run(sub.params(table[pt["set"]: pt["set"] + 1, :n], n_steps=n), sub.seeds())["stream_words"][a])
    rs = np.random.RandomState(int(sub.seeds()[a]))
    rs.randint(0, 2**32, size=words - 2, dtype=np.uint32)
    assert rs.random_sample() == pt["u"]
