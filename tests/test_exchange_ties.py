"""GPU: the sweep kernels under replica exchange on beta tables crafted to put the pair's uniform next to its swap probability and a
chain's uniform next to its acceptance probability at beta(step) * ladder[rung] (tests/exchange_tie_util.py; the oracle's side is pinned on
the CPU by tests/test_exchange_ties_host.py).  Everything is bit for bit, bracketed and with MCQ_FLAG_EXACT_EXP.

ASSUMPTION of the tie points, as in tests/test_near_ties.py: the device's float64 exp and glibc's agree within 1 ulp at the crafted
arguments.  The ties stand 2 or 3 ulp from the uniform, the near misses at 8."""
import numpy as np
import pytest

import mcq_amd
from oracle import oracle
from tests import exchange_tie_util as xt
from tests import near_tie_util as nt
from tests import util

abi = mcq_amd.abi
pytestmark = pytest.mark.gpu
NAMES = [c.name for c in xt.CASES]
EX_FIELDS = ("exchange_rung", "n_exchanges")
_oracle_runs = {}


def _oracle(case, table):
    """The oracle's run of a case under its crafted table: computed once, shared, left unchanged."""
    if case.name not in _oracle_runs:
        _oracle_runs[case.name] = oracle.run(case.params(table), case.seeds(), trace=case.trace, fast=True, n_threads=8)
    return _oracle_runs[case.name]


def exchange_equals_the_oracle_next_to_exp(name, row=None):
    """Every output is the oracle's, swap for swap and tie for tie, and the ties are the crafted ones, on the chains they were crafted for.
    `row` (tests/test_philox_ties.py): the row of SWEEP_TABLE the launch must take, as (MODE, G, NT, NC), on the stream the case names."""
    case = xt.CASES_BY_NAME[name]
    table, points = xt.crafted(name)
    xt.check_plan_was_met(case, points)
    seeds, crafted = case.seeds(), nt.expected_near_ties(case, points)
    want = _oracle(case, table)
    np.testing.assert_array_equal(want["near_ties"], crafted, err_msg=f"{name}: the oracle's own count (tests/test_exchange_ties_host.py)")
    assert int(want["n_exchanges"].sum()) > 0
    v = mcq_amd._lib.sweep_variant(case.params(table))
    assert v["EXCH"] and v["PHILOX"] == (case.rng == "philox") and (not case.lanes or v["G"] == case.lanes), (name, v)
    assert row is None or tuple(int(v[k]) for k in ("MODE", "G", "NT", "NC")) == row, (name, v)
    for flags, how in ((0, "bracketed"), (abi.FLAG_EXACT_EXP, "exact exp")):
        what = f"{name} {how}"
        got, _ = mcq_amd._lib.run_host(case.params(table, flags=flags), seeds, trace=case.trace)
        try:
            assert "near_ties" in util.RESULT_FIELDS
            util.assert_results_equal(got, want, what, trace=case.trace is True)
            for k in EX_FIELDS + ("near_ties",):
                np.testing.assert_array_equal(got[k], want[k], err_msg=f"{what}: {k} per chain")
        except AssertionError as e:
            raise AssertionError(f"{e}\n{what}: {nt.first_difference(got, want, points, trace=case.trace)}") from None
        total = int(got["near_ties"].sum())
        assert total != 0 and total == int(crafted.sum()), f"{what}: {total} near ties, {int(crafted.sum())} crafted"
        np.testing.assert_array_equal(got["near_ties"], crafted, err_msg=f"{what}: near ties per chain vs the crafted counts")
        if case.trace is True:
            for pt in xt.step_points(points):
                assert nt.accept_bit(got, pt["chain"], pt["step"]) == int(pt["accept"]), (what, pt)


@pytest.mark.parametrize("name", NAMES)
def test_exchange_equals_the_oracle_next_to_exp(name):
    exchange_equals_the_oracle_next_to_exp(name)
