"""Every instantiation of mcq_sweep_kernel a launch can take (the reachable rows of SWEEP_TABLE, csrc/mcq_hip.hip) against the CPU oracle,
bit for bit, through the C-ABI: one test per row, over the row's cases of tests/variant_cases.py -- the smallest and the largest N of the
row, ragged chain counts, lengths that end inside every block.  tests/test_variant_cases.py (CPU) holds the table complete; here the
device confirms that a case runs the row it names and the results are compared chain by chain.  The two rows nothing selects
(test_sweep_variant.KNOWN_UNREACHED) have no test: no launch runs them."""
import numpy as np
import pytest

import mcq_amd
from oracle import oracle
from tests import util
from tests import variant_cases as vc

pytestmark = pytest.mark.gpu
STAT_FIELDS = ("step_sum", "step_sumsq", "step_accepted", "step_count")


@pytest.mark.parametrize("row", vc.reachable_rows(), ids=vc.row_id)
def test_row_equals_the_oracle(row):
    cases = vc.cases_of(row)
    assert cases
    for i, c in cases:
        what = f"row {vc.row_id(row)} case {i}: {c}"
        p, seeds = vc.build(c)
        assert vc.variant_of(p) == row, what  # on this device: the launch below runs the kernel the test is named for
        n_steps, reduced = c["steps"], c["trace"] == "reduced"
        # the naive and the fast oracle in turn (the fast one for the cases whose naive run takes seconds: test_variant_cases holds the two together)
        want = oracle.run(p, seeds, n_threads=8, fast=bool(i & 1) or vc.heavy(row, c))
        got, _ = mcq_amd._lib.run_host(p, seeds, trace=c["trace"])
        util.assert_results_equal(got, want, what, trace=not reduced)
        if reduced:  # per schedule set, against the sums of the oracle's full trace
            n_sets = len(c["sched"])
            cps = c["chains"] // n_sets
            for t in range(n_sets):
                st = mcq_amd.jobs.stats_from_trace({f: v[t * cps:(t + 1) * cps] for f, v in want.items()}, n_steps)
                for f in STAT_FIELDS:
                    np.testing.assert_array_equal(got[f][t] if n_sets > 1 else got[f], st[f], err_msg=f"{what}: {f} of set {t}")
        if c["exch"]:
            for f in ("exchange_rung", "n_exchanges"):
                np.testing.assert_array_equal(got[f], want[f], err_msg=f"{what}: {f}")
            assert got["n_exchanges"].sum() > 0, what
        assert got["near_ties"].sum() == 0 and want["near_ties"].sum() == 0, what
        # (assert_results_equal compared hist_len and steps_executed with the oracle's) the shape the case was chosen for
        assert vc.broken_conditions(row, c, got) == [], what
        stopped = got["hist_len"] < n_steps + 1
        if row[2]:
            assert stopped.any() and ((~stopped).any() or c["N"] == 2), what
            assert (got["steps_executed"][~stopped] == n_steps).all(), what
        else:
            assert not stopped.any() and (got["steps_executed"] == n_steps).all(), what
