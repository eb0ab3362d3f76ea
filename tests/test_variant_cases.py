"""CPU-only: the case table of tests/variant_cases.py against the library's selection and the oracle.  Every reachable row of SWEEP_TABLE
has its cases, every case selects the row it is filed under, and the oracle's result of a case has what the case was chosen for -- so
that tests/test_every_variant.py, which runs the table on the GPU, compares every instantiation a launch can take, and a row added to
the table in csrc/mcq_hip.hip without a case fails here."""
import numpy as np
import pytest

import mcq_amd
from oracle import oracle
from tests import util
from tests import variant_cases as vc
from tests.test_sweep_variant import KNOWN_UNREACHED, _table_rows

ROWS = vc.reachable_rows()


def test_the_table_names_every_reachable_row():
    assert {r for r, _ in vc.CASES} == set(_table_rows()) - KNOWN_UNREACHED
    assert len(ROWS) == 131 and set(vc.LARGE_ROWS) <= set(ROWS)
    assert len({c["seed"] for _, c in vc.CASES}) == len(vc.CASES)


def _ends(ns):
    return {min(ns), max(ns)} | ({3} if min(ns) == 2 and 3 in ns else set())


@pytest.mark.parametrize("row", ROWS, ids=vc.row_id)
def test_cases_of_a_row(row):
    assert mcq_amd._lib.lib().mcq_device_simds() == 1024  # the device the table was derived for; the selection looks at nothing else of it
    G, cases = row[1], [c for _, c in vc.cases_of(row)]
    per_wave = 64 // G
    for c in cases:
        what = str(c)
        p, seeds = vc.build(c)
        assert vc.variant_of(p) == row, what
        assert c["steps"] >= 300 and c["steps"] % 16 != 0, what
        assert c["lanes"] == G and (c["flags"] == vc.CNT) == bool(row[11]) and (c["trace"] == "reduced") == bool(row[4]), what
        assert c["trace"] in (True, "reduced"), what  # a full trace wherever the row writes one
        if row in vc.LARGE_ROWS:
            # the smallest count that selects the row: one wavefront of chains fewer takes another one
            assert c["chains"] == vc.LARGE_ROWS[row] and vc.variant_of(vc.build(c, chains=c["chains"] - per_wave)[0]) != row, what
            assert vc.variant_of(vc.build(c, chains=c["chains"] - 1)[0]) != row, what
        else:
            assert c["chains"] <= vc.MAX_CHAINS and c["chains"] > per_wave, what
        if c["exch"]:
            assert c["chains"] % c["exch"][1] == 0, what
        elif len(c["sched"]) > 1:
            assert (c["chains"] // len(c["sched"])) % (32 if G == 2 else 16) == 0, what
        else:
            assert c["chains"] % per_wave != 0, what  # a partially filled wavefront
        # the oracle alone: the fast form everywhere, the naive one beside it (on the first chain or ladder of the heavy cases)
        fast = oracle.run(p, seeds, n_threads=8, fast=True)
        assert vc.broken_conditions(row, c, fast) == [], what
        q, s = vc.build(c, chains=vc.prefix_chains(c)) if vc.heavy(row, c) else (p, seeds)
        naive, head = oracle.run(q, s, n_threads=8), {k: v[: len(s)] for k, v in fast.items()}
        util.assert_results_equal(naive, head, what)
        if c["exch"]:
            for f in ("exchange_rung", "n_exchanges"):
                np.testing.assert_array_equal(naive[f], head[f], err_msg=f"{what}: {f}")
    # both ends of the row's N (and N = 3 besides N = 2), per ladder shape where the row exchanges
    shapes = sorted({c["exch"] for c in cases}) if row[7] else [None]
    for e in shapes:
        group = [c for c in cases if c["exch"] == e]
        single = [c for c in group if len(c["sched"]) == 1]
        ns = vc.selecting_sizes(row, (single or group)[0])
        plain = [c for c in group if (c["Q"] is None) == (ns[c["N"]] is None)]  # Q = N^2 wherever that selects the row
        assert {c["N"] for c in plain} == _ends(ns), (e, sorted(ns))
        assert len(plain) == len(group) or row[10]
        if row[10]:  # SLIM: another queen count besides, where the row takes one
            takes = any(vc.variant_of(vc.build(dict(single[0], N=N, Q=N * N + 13, init="random"))[0]) == row for N in ns)
            assert any(c["Q"] for c in group) == takes
    if row[7]:  # EXCH: a ladder as wide as the lanes allow, and ladders of two
        assert {e[1] for e in shapes} == {min(16, per_wave), 2}
    if row[4] and row not in vc.LARGE_ROWS:  # REDUCED: schedule sets of their own init modes, and a single schedule with a ragged count
        assert any(len(c["sched"]) > 1 and len(set(c["inits"])) > 1 for c in cases) and any(len(c["sched"]) == 1 for c in cases)
