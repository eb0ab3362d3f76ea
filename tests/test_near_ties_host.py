"""CPU only: the oracle's near-tie counter and accept decision on beta tables crafted to put the uniform next to exp(-beta dE)
(tests/near_tie_util.py), and Checkpoint.merge on near-tie counts that are not zero.  The oracle is what the kernels are compared with
(tests/test_near_ties.py); its counter had never counted either, so it is pinned here against the crafted counts and against the decision
recomputed in Python from (u, beta, dE)."""
import math

import numpy as np
import pytest

import mcq_amd
from oracle import oracle
from tests import near_tie_util as nt

abi = mcq_amd.abi
NAMES = [c.name for c in nt.CASES]


def oracle_counts_the_crafted_ties_and_decides_as_recomputed(name):
    """(tests/test_philox_ties_host.py runs the same on the Philox cases.)"""
    case = nt.CASES_BY_NAME[name]
    table, points = nt.crafted(name)
    nt.check_plan_was_met(case, points)
    seeds, want = case.seeds(), nt.expected_near_ties(case, points)
    runs = {"oracle": oracle.run(case.params(table, trace=True), seeds, n_threads=4),
            "fast oracle": oracle.run(case.params(table, trace=True), seeds, n_threads=4, fast=True)}
    for what, res in runs.items():
        np.testing.assert_array_equal(res["near_ties"], want, err_msg=f"{name}: {what}: near_ties per chain")
        for pt in points:
            c, s = pt["chain"], pt["step"]
            assert table[pt["set"], s] == pt["beta"]
            if pt["kind"] == "behind":
                assert int(res["steps_executed"][c]) <= s, f"{name}: {what}: chain {c} was to have stopped before step {s}"
                continue
            assert int(res["hist_len"][c]) > s + 1, f"{name}: {what}: chain {c} does not reach the crafted step {s}"
            acc = u_below = pt["u"] < math.exp(-pt["beta"] * pt["dE"])
            assert nt.accept_bit(res, c, s) == int(acc), f"{name}: {what}: chain {c} step {s} ({pt['kind']}, {pt['ulps']:+d} ulp): accept bit"
            assert int(res["energy_hist"][c, s + 1]) - int(res["energy_hist"][c, s]) == (pt["dE"] if u_below else 0), (name, what, c, s)
    for k in runs["oracle"]:
        np.testing.assert_array_equal(runs["oracle"][k], runs["fast oracle"][k], err_msg=f"{name}: fast oracle vs oracle: {k}")
    if case.trace is not True:  # the counter does not depend on what is traced
        np.testing.assert_array_equal(oracle.run(case.params(table), seeds, trace=case.trace, n_threads=4)["near_ties"], want)
    control = oracle.run(case.params(case.base_table()), seeds, trace=case.trace, n_threads=4)
    assert int(control["near_ties"].sum()) == 0, f"{name}: the uncrafted table ties by itself"
    if case.patience is not None:  # the ties behind the stops are real: without early stopping the chains reach them and they count
        free = oracle.run(case.params(table, patience=None), seeds, n_threads=4)
        behind = [pt for pt in points if pt["kind"] == "behind"]
        assert behind and all(int(free["near_ties"][pt["chain"]]) >= 1 and nt.accept_bit(free, pt["chain"], pt["step"]) == 1 for pt in behind)
        assert int(free["near_ties"].sum()) > int(want.sum())


@pytest.mark.parametrize("name", NAMES)
def test_oracle_counts_the_crafted_ties_and_decides_as_recomputed(name):
    oracle_counts_the_crafted_ties_and_decides_as_recomputed(name)


def test_crafted_uniforms_are_the_streams_words():
    """The u of a crafted point is NumPy's own random_sample at that place of the chain's stream."""
    case = nt.CASES_BY_NAME["board6_g4"]
    table, points = nt.crafted(case.name)
    pt = points[0]
    p = abi.make_params(case.N, pt["step"] + 1, "random", case.base_schedules()[0], 1, mcmc_type=case.mode)
    tab = np.ascontiguousarray(table[pt["set"]: pt["set"] + 1, : pt["step"] + 1])
    p._schedules, p.beta_table = None, tab.ctypes.data
    seed = int(case.seeds()[pt["chain"]])
    words = int(oracle.run(p, np.array([seed], dtype=np.uint32))["stream_words"][0])
    rs = np.random.RandomState(seed)
    rs.randint(0, 2**32, size=words - 2, dtype=np.uint32)
    assert rs.random_sample() == pt["u"]


def test_checkpoint_merge_adds_near_ties_up():
    Checkpoint = mcq_amd.checkpoint.Checkpoint
    c = Checkpoint(4, "board", 30, np.array([1, 2, 3], dtype=np.uint32), schedule_params={"type": "constant", "beta_const": 1.0})
    seg = lambda e0, e1, ties: {"initial_energy": np.array(e0), "final_energy": np.array(e1), "best_energy": np.array(e1),  # noqa: E731
                                "steps_to_best": np.array([1, 1, 1]), "n_accepted": np.array([2, 2, 2]), "near_ties": np.array(ties, dtype=np.int64)}
    c.merge(seg([9, 9, 9], [7, 7, 7], [0, 2, 1]), 10)
    assert c.near_ties.tolist() == [0, 2, 1]
    c.merge(seg([7, 7, 7], [6, 6, 6], [3, 0, 1]), 10)
    c.merge(seg([6, 6, 6], [5, 5, 5], [0, 0, 5]), 10)
    assert c.near_ties.dtype == np.int64 and c.near_ties.tolist() == [3, 2, 7]


def test_checkpoint_keeps_near_ties_through_a_file(tmp_path):
    Checkpoint = mcq_amd.checkpoint.Checkpoint
    c = Checkpoint(4, "board", 30, np.array([1, 2], dtype=np.uint32), schedule_params={"type": "constant", "beta_const": 1.0})
    c.merge({"initial_energy": np.array([9, 9]), "final_energy": np.array([7, 8]), "best_energy": np.array([7, 8]), "steps_to_best": np.array([1, 2]),
             "n_accepted": np.array([2, 2]), "near_ties": np.array([4, 0], dtype=np.int64)}, 10)
    path = str(tmp_path / "c.npz")
    c.save(path)
    assert Checkpoint.load(path).near_ties.tolist() == [4, 0]


def test_checkpoint_without_the_count_stays_without():
    """A checkpoint that stands mid-run without near_ties (one saved before the count was kept) does not pass the later segments' ties
    off as the run's."""
    Checkpoint = mcq_amd.checkpoint.Checkpoint
    c = Checkpoint(4, "board", 30, np.array([1, 2], dtype=np.uint32), schedule_params={"type": "constant", "beta_const": 1.0})
    seg = {"initial_energy": np.array([9, 9]), "final_energy": np.array([7, 8]), "best_energy": np.array([7, 8]), "steps_to_best": np.array([1, 2]),
           "n_accepted": np.array([2, 2])}
    c.merge(seg, 10)
    assert c.near_ties is None
    c.merge(dict(seg, initial_energy=np.array([7, 8]), near_ties=np.array([1, 1], dtype=np.int64)), 10)
    assert c.near_ties is None
