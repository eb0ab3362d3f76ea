"""GPU: the sweep kernel's accept decision over the whole range of beta dE (tests/accept_range_util.py; the oracle's side and the Python
truth are pinned on the CPU by tests/test_accept_range_host.py): probabilities next to 1, probabilities so small that the 1/2 of the float32
bracket's half-width is all of it (down to a uniform below 2^-27), negative beta, and zeros, NaN, infinities, denormals and beta values
whose float32 image underflows or overflows.  Ten launches, each bracketed and with MCQ_FLAG_EXACT_EXP, bit for bit against the oracle.

The ties of the high region and of the negative row rest on the assumption of tests/test_near_ties.py (the device's exp and glibc's agree
within 1 ulp at these arguments).  Every other crafted point stands 1000 ulp or more from its uniform, or is a special value: an accept bit
that differs there is a kernel bug."""
import numpy as np
import pytest

import mcq_amd
from oracle import oracle
from tests import accept_range_util as ar
from tests import near_tie_util as nt
from tests.test_near_ties import _assert_equal

abi = mcq_amd.abi
pytestmark = pytest.mark.gpu
NAMES = [c.name for c in ar.CASES]
_oracle_runs = {}


def _oracle(case, table):
    """The oracle's run of a case under its crafted table: once per process, shared, left unchanged (for the reduced-trace case the run
    with the full trace plus the per-set sums of that trace)."""
    if case.name not in _oracle_runs:
        res = oracle.run(case.params(table, trace=True), case.seeds(), trace=True, n_threads=8)
        if case.trace == "reduced":
            res.update(nt.reduced_from_trace(res, case.n_steps, case.n_sets))
        _oracle_runs[case.name] = res
    return _oracle_runs[case.name]


def _first_crafted_difference(got, want, points):
    """The first crafted or special point, in step order, that the device or the oracle decides against the Python truth, and which of them."""
    for pt in sorted(points, key=lambda pt: (pt["step"], pt["chain"])):
        truth, dev, orc = int(pt["accept"]), nt.accept_bit(got, pt["chain"], pt["step"]), nt.accept_bit(want, pt["chain"], pt["step"])
        if dev != truth or orc != truth:
            wrong = " and ".join(w for w, b in (("the device", dev), ("the oracle", orc)) if b != truth)
            return (f"first crafted point that {wrong} decided against the truth: chain {pt['chain']}, step {pt['step']}: {ar.describe(pt)}, dE {pt['dE']}, "
                    f"u {pt['u']!r}, beta {pt['beta']!r}, truth {truth}, device {dev}, oracle {orc}")
    return None


@pytest.mark.parametrize("name", NAMES)
def test_sweep_decides_as_the_oracle_over_the_whole_range(name):
    case = ar.CASES_BY_NAME[name]
    table, points = ar.crafted(name)
    ar.check_plan_was_met(case, points)
    seeds, crafted = case.seeds(), ar.expected_near_ties(case, points)
    want = _oracle(case, table)
    np.testing.assert_array_equal(want["near_ties"], crafted, err_msg=f"{name}: the oracle's own count (tests/test_accept_range_host.py)")
    v = mcq_amd._lib.sweep_variant(case.params(table))
    assert tuple(int(v[k]) for k in abi.SWEEP_VARIANT_FIELDS) == case.row, (name, v)
    for flags, how in ((0, "bracketed"), (abi.FLAG_EXACT_EXP, "exact exp")):
        got, _ = mcq_amd._lib.run_host(case.params(table, flags=flags), seeds, trace=case.trace)
        try:
            _assert_equal(got, want, case, points, f"{name} {how}")
        except AssertionError as e:
            raise AssertionError(f"{e}\n{_first_crafted_difference(got, want, points) if case.trace is True else ''}") from None
        assert int(got["near_ties"].sum()) == int(crafted.sum()) == 8
        np.testing.assert_array_equal(got["near_ties"], crafted, err_msg=f"{name} {how}: near ties per chain vs the crafted counts")
        if case.trace is True:
            wrong = _first_crafted_difference(got, want, points)
            assert wrong is None, f"{name} {how}: {wrong}"
