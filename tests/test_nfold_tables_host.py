"""CPU-only: the n-fold way in host code (mcq_nfold_host, mcq_nfold3d_host) against its NumPy restatements on weight rows and clocks of
the CALLER's (tests/nfold_tables_util.py), which nfold.weight_tables and nfold.clock_tables never build: every family under both clocks
and three segments on every field, the history included, at boards N = 3, 5, 9, 13 and at (N, Q) = (3, 4), (4, 16), (5, 30) with input
bytes >= N; what these runs cover, asserted from the restatements' traces; the closed form under the row [1] and the clock of ones at
every N = 2 .. 32 and at seven cubes; and runs cut at every segment boundary under rows that change character between segments.

The restatements recount everything behind every event, so events are cut, never families or shapes: the families of tu.HEAVY run one
step per segment; `rand`, whose every step fires 4096 events for good, carries a need aimed so that the chain sleeps through two segments
and fires in the last 40 units of the third, under each of its three rows in turn; `altzero` fires in the last 40 units of its first
segment, sleeps through the zero row and climbs under the third."""
import functools

import numpy as np
import pytest

import mcq_amd
from tests import nfold3d_util as n3
from tests import nfold_tables_util as tu
from tests import nfold_util as nu
from tests import quench3d_util as q3
from tests import quench_util as qu

abi = mcq_amd.abi
nfold = mcq_amd.nfold
SEGS = 3
BOARDS = (3, 5, 9, 13)
CUBES = ((3, 4), (4, 16), (5, 30))
FAMILIES = tuple(tu.rows(SEGS, 128))
CLOCKS = tuple(tu.clocks())
TICKS = 40


def _plan(family, big):
    """(chains, steps per segment) of a family: four chains and six steps for the light ones, one step and fewer chains where events are many."""
    if family not in tu.HEAVY:
        return 4, 6
    return (1 if big else 2), 1


@functools.lru_cache(maxsize=None)
def _board_run(N, family, clock):
    """[(what, placements, seeds, rows, steps, need_in, the restatement's result, its traces)] of a family at N: computed once."""
    n, steps = _plan(family, N >= 13)
    s = qu.random_boards(N, 4, 100 + N, over=True)[:n]
    seeds = abi.seeds_for(4000000000 + N, 4)[:n]
    ck = tu.clocks()[clock]
    rows = tu.rows(SEGS, abi.MAX_NFOLD_TABLE)[family]
    runs = []
    for turn in range(SEGS if family == "rand" else 1):
        t = np.ascontiguousarray(np.roll(rows, -turn, axis=0))
        need = None
        if family in tu.NEVER_QUIET:
            upto = SEGS if family == "rand" else 1
            need = np.array([tu.aimed_need(tu.board_weights(N, b, t[:upto]), TICKS) for b in s], dtype=np.uint64)
            assert int(need.max()) < 1 << abi.NFOLD_NEED_BITS
        traces = []
        want = nu.nfold_many(N, s, seeds, t, steps, ck, need_in=need, traces=traces)
        runs.append((f"N = {N}, {family}, {clock}, rows turned by {turn}", s, seeds, t, steps, need, want, traces))
    return runs


@functools.lru_cache(maxsize=None)
def _cube_run(N, Q, family, clock):
    n, steps = _plan(family, N >= 5)
    s = q3.random_placements(N, 4, 100 + N, Q=Q, over=True)[:n]
    assert (s >= N).any()
    seeds = abi.seeds_for(4000000000 + N, 4)[:n]
    ck = tu.clocks()[clock]
    rows = tu.rows(SEGS, abi.MAX_NFOLD3D_TABLE)[family]
    runs = []
    for turn in range(SEGS if family == "rand" else 1):
        t = np.ascontiguousarray(np.roll(rows, -turn, axis=0))
        need = None
        if family in tu.NEVER_QUIET:
            upto = SEGS if family == "rand" else 1
            need = np.array([tu.aimed_need(tu.queen_weights(N, p, t[:upto]), TICKS) for p in s], dtype=np.uint64)
            assert int(need.max()) < 1 << abi.NFOLD3D_NEED_BITS
        traces = []
        want = n3.nfold_many(N, s, seeds, t, steps, ck, Q=Q, need_in=need, traces=traces)
        runs.append((f"(N, Q) = ({N}, {Q}), {family}, {clock}, rows turned by {turn}", s, seeds, t, steps, need, want, traces))
    return runs


def _events(runs):
    """[(U, W, lo, hi, zero_before)] of every event of the runs, boards (trace entries 5 ..) or cubes (6 ..)."""
    return [ev[-5:] if len(ev) == 10 else (ev[6], ev[7]) + ev[8:] for run in runs for tr in run[-1] for ev in tr]


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("N", BOARDS)
def test_board_host_code_equals_the_restatement(N, family):
    for clock in CLOCKS:
        for what, s, seeds, t, steps, need, want, traces in _board_run(N, family, clock):
            got = nfold.nfold_states_host(N, s, seeds, t, steps, clock=tu.clocks()[clock], need_in=need, hist=True)
            nu.assert_equal(got, want, what)
            assert got["energy_hist"].shape == (len(s), SEGS + 1) and got["need_out"].dtype == np.uint64


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("N,Q", CUBES)
def test_cube_host_code_equals_the_restatement(N, Q, family):
    for clock in CLOCKS:
        for what, s, seeds, t, steps, need, want, traces in _cube_run(N, Q, family, clock):
            got = nfold.nfold_queens_host(N, s, seeds, t, steps, Q=Q, clock=tu.clocks()[clock], need_in=need, hist=True)
            n3.assert_equal(got, want, what)
            assert got["energy_hist"].shape == (len(s), SEGS + 1) and (got["flags"] == 0).all()


def _covered(kind, shapes, run):
    """The coverage conditions over the restatement's runs, asserted; the counts are printed per family."""
    small = dict(first=0, last=0, zero_before=0, events=0)
    for family in FAMILIES:
        count = dict(events=0, first=0, last=0, zero_before=0, uphill=0)
        for shape in shapes:
            for clock in CLOCKS:
                runs = run(*shape, family, clock)
                evs = _events(runs)
                assert all(lo <= U < hi <= W for U, W, lo, hi, _ in evs)
                fired = sum(int((r[6]["events_out"] > 0).sum()) for r in runs)
                # the rows with T[0] = 0 and weight on few distances find nothing to move at the smallest shape under some clocks
                assert fired > 0 or (family in ("only3", "up_only") and shape == shapes[0]), (kind, shape, family, clock)
                count["events"] += len(evs)
                count["first"] += sum(U == lo for U, W, lo, hi, _ in evs)
                count["last"] += sum(U == hi - 1 for U, W, lo, hi, _ in evs)
                count["zero_before"] += sum(bool(z) for *_, z in evs)
                count["uphill"] += sum(int(r[6]["n_uphill"].sum()) for r in runs)
                if family == "ones":
                    assert all(U == lo == hi - 1 for U, W, lo, hi, _ in evs), (kind, shape, clock)
                if family == "altzero":
                    for *_, want, traces in runs:
                        hist = want["energy_hist"]
                        assert (hist[:, 1] == hist[:, 2]).all(), (kind, shape, clock)
                        for tr in traces:
                            segs = {ev[0] for ev in tr}
                            assert segs == {0, 2}, (kind, shape, clock, segs)
        print(f"{kind} {family}: {count}")
        assert count["events"] > 0
        if family in ("rising", "clip"):
            assert count["uphill"] > 0, family
        if family in tu.SMALL:
            for k in ("first", "last", "zero_before", "events"):
                small[k] += count[k]
    print(f"{kind}, the small-weight families {tu.SMALL}: {small}")
    assert small["first"] > 0 and small["last"] > 0 and small["zero_before"] > 0, small


def test_what_the_board_runs_cover():
    _covered("boards", tuple((N,) for N in BOARDS), _board_run)


def test_what_the_cube_runs_cover():
    _covered("full_3d", CUBES, _cube_run)


@pytest.mark.parametrize("N", tuple(range(2, 33)))
def test_board_closed_form_under_ones_and_the_unit_clock(N):
    n, steps = 4, 5
    s = qu.random_boards(N, n, 200 + N, over=True)
    seeds = abi.seeds_for(3000000000 + N, n)
    M = N * N * (N - 1)
    want, _ = tu.boards_after(N, s, seeds, steps * SEGS)
    got = nfold.nfold_states_host(N, s, seeds, tu.rows(SEGS, abi.MAX_NFOLD_TABLE)["ones"], steps, clock=tu.clocks()["unit"])
    assert (got["events_out"] == steps * SEGS).all() and (got["need_out"] == M).all() and (got["weight_out"] == M).all()
    np.testing.assert_array_equal(got["state"], want)


@pytest.mark.parametrize("N,Q", ((2, 3), (3, 4), (6, 36), (12, 37), (13, 11), (20, 7), (32, 5)))
def test_cube_closed_form_under_ones_and_the_unit_clock(N, Q):
    n, steps = 4, 5
    s = q3.random_placements(N, n, 200 + N, Q=Q, over=True)
    seeds = abi.seeds_for(3000000000 + N, n)
    M = Q * (N ** 3 - Q)
    want, _ = tu.queens_after(N, Q, s, seeds, steps * SEGS)
    got = nfold.nfold_queens_host(N, s, seeds, tu.rows(SEGS, abi.MAX_NFOLD3D_TABLE)["ones"], steps, Q=Q, clock=tu.clocks()["unit"])
    assert (got["flags"] == 0).all()
    assert (got["events_out"] == steps * SEGS).all() and (got["need_out"] == M).all() and (got["weight_out"] == M).all()
    np.testing.assert_array_equal(got["state"], want)


def _cut_equals_whole(run, s, seeds, tabs, clock):
    S = len(tabs)
    whole = run(s, seeds, tabs, 0, clock, None, None)
    for cut in range(S + 1):
        a = run(s, seeds, tabs[:cut], 0, clock, None, None)
        b = run(a["state"], seeds, tabs[cut:], cut, clock, a["need_out"], a["events_out"])
        for k in ("state", "energy_out", "events_out", "need_out"):
            np.testing.assert_array_equal(b[k], whole[k], err_msg=f"cut {cut}: {k}")
        if cut < S:
            np.testing.assert_array_equal(b["weight_out"], whole["weight_out"])
        np.testing.assert_array_equal(np.concatenate([a["energy_hist"], b["energy_hist"][:, 1:]], axis=1), whole["energy_hist"])
        np.testing.assert_array_equal(a["n_uphill"] + b["n_uphill"], whole["n_uphill"])
        np.testing.assert_array_equal(a["n_flat"] + b["n_flat"], whole["n_flat"])
        first = a["best_energy"] <= b["best_energy"]
        np.testing.assert_array_equal(np.where(first, a["best_energy"], b["best_energy"]), whole["best_energy"])
        np.testing.assert_array_equal(np.where(first, a["best_step"], b["best_step"] + cut), whole["best_step"])
        np.testing.assert_array_equal(np.where(first[:, None], a["best_state"], b["best_state"]), whole["best_state"])
    return whole


@pytest.mark.parametrize("clock", CLOCKS)
@pytest.mark.parametrize("family", ("altzero", "rand"))
def test_a_board_run_cut_at_every_segment_boundary_is_the_unbroken_run(family, clock):
    N, n, S = 5, 5, 4
    tabs = tu.rows(S, abi.MAX_NFOLD_TABLE)[family]
    ck = tu.clocks()[clock]
    whole = _cut_equals_whole(lambda s, sd, t, first, c, need, ev: nfold.nfold_states_host(N, s, sd, t, 1, first_seg=first, clock=c, need_in=need,
                                                                                            events_in=ev, hist=True),
                              qu.random_boards(N, n, 70 + N), abi.seeds_for(910 + N, n), tabs, ck)
    assert int(whole["events_out"].min()) > S


@pytest.mark.parametrize("clock", CLOCKS)
@pytest.mark.parametrize("family", ("altzero", "rand"))
def test_a_cube_run_cut_at_every_segment_boundary_is_the_unbroken_run(family, clock):
    N, Q, n, S = 4, 16, 3, 4
    tabs = tu.rows(S, abi.MAX_NFOLD3D_TABLE)[family]
    ck = tu.clocks()[clock]
    whole = _cut_equals_whole(lambda s, sd, t, first, c, need, ev: nfold.nfold_queens_host(N, s, sd, t, 1, Q=Q, first_seg=first, clock=c, need_in=need,
                                                                                            events_in=ev, hist=True),
                              q3.random_placements(N, n, 70 + N, Q=Q), abi.seeds_for(910 + N, n), tabs, ck)
    assert int(whole["events_out"].min()) > S
