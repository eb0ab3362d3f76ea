"""CPU-only: tabu search of full_3d placements in host code (mcq_tabu3d_host) against its NumPy restatement (tests/tabu3d_util.py, a brute
force over all pairs of a conflicting queen and a free cell) on every output, histories and tabu_out included: N = 2 .. 6 with Q = N^2,
the shapes with one or two free cells and with two or three queens, one case in each of the other two shapes of the kernel; that the
compared runs move, rise, aspire and stall (from the restatement's traces); the tenure terms alone and the cap of the tenure in a dense
cube; the placements at the ends of the kernel's packed key; n_iters = 0; a run cut at several points; best_state against the full_3d
quench; a repeated placement among sound ones; first_iter on both sides of 2^32; every refusal; the LDS formula; the layout of the
mcq_tabu3d block; the source list."""
import ctypes
import functools
import os
import subprocess
import tempfile

import numpy as np
import pytest

import mcq_amd
from tests import quench3d_util as q3
from tests import tabu3d_util as t3

abi = mcq_amd.abi
quench = mcq_amd.quench
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TENURES = ((0, 0, 0), (3, 4, 0), (0, 9, 10))
ITERS = 40
# (N, Q): Q = N^2 (None) at N = 2 .. 6, and two or three queens and one or two free cells at N = 2, 3, 4
SHAPES = tuple((N, None) for N in range(2, 7)) + tuple((N, Q) for N in (2, 3, 4) for Q in (2, 3, N ** 3 - 2, N ** 3 - 1))
ALL = dict(hist=True, tabu_out=True)


@functools.lru_cache(maxsize=None)
def _case(N, Q, ti):
    """(placements, seeds, keywords, the restatement's result) of one comparison; computed once and shared, never changed."""
    n = 3
    tenure, tenure_rand, tenure_conf = TENURES[ti]
    s = q3.random_placements(N, n, 100 * N + (Q or 0) + ti, Q=Q, over=True)
    seeds = abi.seeds_for(5 + N + ti, n)
    tin = np.random.RandomState(N + ti).randint(0, 6, size=(n, N ** 3)).astype(np.uint16) if ti else None
    kw = dict(Q=Q, tenure=tenure, tenure_rand=tenure_rand, tenure_conf=tenure_conf, tabu_in=tin)
    return s, seeds, kw, t3.tabu_many(N, s, seeds, ITERS, **kw)


def test_the_compared_runs_move_rise_aspire_and_stall():
    """The condition on the inputs of test_host_code_equals_the_restatement, from the restatement's traces of those very cases."""
    assert set(t3.FIELDS) == set(quench.FIELDS_TABU3D) and t3.KEY_WORD == 8 and t3.SPAN == abi.MAX_TABU3D_SPAN
    total = dict()
    for N, Q in SHAPES:
        for ti in range(len(TENURES)):
            s, seeds, kw, want = _case(N, Q, ti)
            tally = t3.tally(want["trace"])
            counted = quench.tabu_queens_host(N, s, seeds, ITERS, **kw)  # the traces are those of the runs the host code makes
            assert tally["moves"] == int(counted["n_moves"].sum()) and tally["uphill"] == int(counted["n_uphill"].sum())
            assert tally["aspired"] == int(counted["n_aspired"].sum()) and tally["stalls"] == int(counted["n_stalled"].sum())
            for k, v in tally.items():
                total[k] = total.get(k, 0) + v
            if Q is None and N >= 4:  # the random-placement group: it walks
                assert 2 * tally["stalls"] <= 3 * ITERS, (N, ti, tally)
    print(total)
    for k in ("moves", "uphill", "aspired", "stalls", "stall_above_0", "on_line", "wrapped_q", "wrapped_t"):
        assert total[k] >= 20, (k, total)
    assert total["moves"] > total["on_line"]  # winners on the moved queen's own lines, and off them


@pytest.mark.parametrize("N,Q", SHAPES)
def test_host_code_equals_the_restatement(N, Q):
    for ti in range(len(TENURES)):
        s, seeds, kw, want = _case(N, Q, ti)
        got = quench.tabu_queens_host(N, s, seeds, ITERS, **ALL, **kw)
        t3.assert_equal(got, want, f"N={N} Q={Q} tenure set {ti}")
        assert set(got) == set(quench.FIELDS_TABU3D) == set(t3.FIELDS)
        n, Qn = s.shape[0], s.shape[1] // 3
        assert got["state"].shape == got["best_state"].shape == (n, 3 * Qn) and got["state"].dtype == np.uint8 and int(got["state"].max()) < N
        assert got["energy_hist"].shape == (n, ITERS + 1) and got["tabu_out"].shape == (n, N ** 3)
        for k, dt in abi.TABU3D_DTYPES.items():
            assert got[k].dtype == dt and (k in ("energy_hist", "tabu_out") or got[k].shape == (n,)), k
        slim = quench.tabu_queens_host(N, s, seeds, 2, **kw)
        assert "energy_hist" not in slim and "tabu_out" not in slim


@pytest.mark.parametrize("N,Q", ((13, 150), (20, 401)))
def test_host_code_equals_the_restatement_in_the_other_shapes(N, Q):
    s = q3.random_placements(N, 1, N, Q=Q, over=True)
    seeds = abi.seeds_for(N, 1)
    tin = np.random.RandomState(N).randint(0, 20, size=(1, N ** 3)).astype(np.uint16)
    kw = dict(Q=Q, tenure=3, tenure_rand=4, tenure_conf=1, tabu_in=tin)
    want = t3.tabu_many(N, s, seeds, 30, **kw)
    t3.assert_equal(quench.tabu_queens_host(N, s, seeds, 30, **ALL, **kw), want, f"N={N} Q={Q}")
    assert t3.tally(want["trace"])["moves"] == 30


def test_the_tenure_terms_each_alone():
    for N, Q, n, iters, kw in ((4, None, 3, 60, dict(tenure=0, tenure_rand=6)), (5, None, 2, 60, dict(tenure=0, tenure_conf=24)),
                               (8, 500, 1, 6, dict(tenure=1, tenure_conf=64)), (3, None, 3, 60, dict(tenure=0, tenure_rand=4095))):
        s, seeds = q3.random_placements(N, n, 80 + N, Q=Q), abi.seeds_for(21 + N, n)
        want = t3.tabu_many(N, s, seeds, iters, Q=Q, **kw)
        t3.assert_equal(quench.tabu_queens_host(N, s, seeds, iters, Q=Q, **ALL, **kw), want, f"N={N} {kw}")
        moves = [tr for chain in want["trace"] for tr in chain if tr["moved"]]
        varied = 1 if Q else 2 if "tenure_conf" in kw else 4  # (in the dense cube every queen conflicts all the time: F = Q)
        assert len(moves) >= 6 and len({tr["L"] for tr in moves}) >= varied, "the tenure never varied"
        if "tenure_conf" in kw:
            assert all(tr["L"] == kw["tenure"] + kw["tenure_conf"] * tr["F"] // 16 for tr in moves) and len({tr["F"] for tr in moves}) >= varied
            assert Q is None or {tr["L"] for tr in moves} == {1 + 4 * 500}
        else:
            assert all(0 <= tr["L"] <= kw["tenure_rand"] for tr in moves)
    # no tenure at all: nothing is ever tabu
    got = quench.tabu_queens_host(5, q3.random_placements(5, 3, 1), abi.seeds_for(2, 3), 50, tenure=0, tabu_out=True)
    assert not got["n_aspired"].any() and not got["n_stalled"].any() and int(got["tabu_out"].max()) <= 1


def test_the_cap_of_the_tenure_in_a_dense_cube():
    """tenure_conf F / 16 alone passes MCQ_MAX_TABU3D_SPAN only with F > 4 095 conflicting queens: N = 17 with 4 500 of its 4 913 cells
    taken, three iterations."""
    N, Q = 17, 4500
    s, seeds = q3.random_placements(N, 1, 5, Q=Q), abi.seeds_for(1, 1)
    want = t3.tabu_many(N, s, seeds, 3, Q=Q, tenure=0, tenure_conf=64)
    got = quench.tabu_queens_host(N, s, seeds, 3, Q=Q, tenure=0, tenure_conf=64, **ALL)
    t3.assert_equal(got, want, "the dense cube")
    moves = [tr for tr in want["trace"][0] if tr["moved"]]
    assert len(moves) == 3 and all(tr["F"] > 4095 and 64 * tr["F"] // 16 > t3.SPAN and tr["L"] == t3.SPAN for tr in moves)
    assert abi.MAX_TABU3D_SPAN == t3.SPAN == (1 << 14) - 1 and int(got["tabu_out"].max()) == t3.SPAN


@pytest.mark.parametrize("N", t3.KEY_N)
def test_the_largest_fall_and_the_largest_rise(N):
    """The ends of delta in the kernel's key, as host code runs them (tests/tabu3d_util.py: key_case; DESIGN.md says how they were derived)."""
    lines = len(t3.star(N)) - 1
    assert lines == {19: 13 * 18, 32: 397}[N]
    for kind in ("fall", "rise"):
        s, seeds, iters, kw, want = t3.key_case(N, kind)
        deltas = [tr["delta"] for tr in want["trace"][0] if tr["moved"]]
        print(N, kind, deltas)
        if kind == "fall":  # the centre queen, attacked along all its lines, to a cell that nothing attacks
            assert deltas[0] == -lines
        else:  # the one open cell is the centre, with every line cell taken: the smallest delta is that of a queen of the longest lines
            assert deltas[0] == t3.KEY_RISE[N] and deltas[0] > 0 and want["n_uphill"][0] >= 1
        t3.assert_equal(quench.tabu_queens_host(N, s, seeds, iters, **ALL, **kw), want, f"N={N} {kind}")


def test_the_largest_rho():
    for N in (4, 32):
        s, seeds, kw, want, (rq, rt) = t3.rho_case(N)
        assert (rq, rt) == (2, N ** 3 - 1)
        tr = want["trace"][0][0]
        oq, _, ot = t3.draw(seeds[0], 0, N, 3, 0)
        assert tr["moved"] and ((tr["q"] - oq) % 3, (tr["t"] - ot) % N ** 3) == (rq, rt)
        t3.assert_equal(quench.tabu_queens_host(N, s, seeds, 2, **ALL, **kw), want, f"N={N}: the largest rho")


def test_no_iterations_is_the_recount():
    for N, Q, n in ((2, 3, 3), (5, None, 4), (13, 100, 2), (32, None, 1)):
        s = q3.random_placements(N, n, 9 + N, Q=Q, over=True)
        tin = np.random.RandomState(N).randint(0, 1 << 16, size=(n, N ** 3)).astype(np.uint16)
        seeds = abi.seeds_for(1, n)
        got = quench.tabu_queens_host(N, s, seeds, 0, Q=Q, tenure=5, first_iter=(1 << 40) + 3, tabu_in=tin, **ALL)
        clamped = np.minimum(s, N - 1)
        np.testing.assert_array_equal(got["state"], clamped)
        np.testing.assert_array_equal(got["best_state"], clamped)
        np.testing.assert_array_equal(got["tabu_out"], tin)
        e = np.array([q3.pairwise_energy(N, b) for b in s])
        for k in ("energy_in", "energy_out", "best_energy"):
            np.testing.assert_array_equal(got[k], e, err_msg=k)
        np.testing.assert_array_equal(got["energy_hist"], e[:, None])
        for k in t3.COUNTERS + ("best_iter", "flags"):
            assert not got[k].any(), k
        floor = e - np.arange(n, dtype=np.int64) + 1  # above, at and below the recount
        low = quench.tabu_queens_host(N, s, seeds, 0, Q=Q, best_floor=floor.astype(np.int32))
        np.testing.assert_array_equal(low["best_energy"], np.minimum(floor, e))
        assert "tabu_out" not in low and not quench.tabu_queens_host(N, s, seeds, 0, Q=Q, tabu_out=True)["tabu_out"].any()


def test_a_cut_run_is_the_unbroken_run():
    for N, Q, n, kw in ((3, None, 5, dict(tenure=2, tenure_rand=3)), (5, None, 6, dict(tenure=4, tenure_rand=2, tenure_conf=8)), (9, 50, 3, dict(tenure=7, tenure_conf=3)),
                        (4, 62, 4, dict(tenure=8192, tenure_rand=4095, tenure_conf=64))):
        s = q3.random_placements(N, n, 40 + N, Q=Q, over=True)
        seeds = abi.seeds_for(9, n)
        tin = np.random.RandomState(N).randint(0, 12, size=(n, N ** 3)).astype(np.uint16)
        whole = quench.tabu_queens_host(N, s, seeds, 150, Q=Q, first_iter=4, tabu_in=tin, **ALL, **kw)
        for cuts in ((7, 1, 142), (75, 75), (1, 148, 1)):
            parts = t3.run_cut(quench.tabu_queens_host, N, s, seeds, cuts, Q=Q, first_iter=4, tabu_in=tin, **ALL, **kw)
            t3.assert_equal(t3.merge(parts), whole, f"N={N}: {cuts} iterations")
        if Q is None:
            assert (whole["best_iter"] > 8).any(), "no chain found its best in the later calls"
            # at another first_iter the pieces are other runs
            assert not np.array_equal(quench.tabu_queens_host(N, s, seeds, 150, Q=Q, first_iter=5, tabu_in=tin, hist=True, **kw)["energy_hist"], whole["energy_hist"])
    # the restatement cut the same way is the restatement unbroken: consequence (b) holds for the rule, not only for the host code
    N, n, kw = 4, 3, dict(tenure=3, tenure_rand=2, tenure_conf=16)
    s, seeds = q3.random_placements(N, n, 44, over=True), abi.seeds_for(10, n)
    whole = t3.tabu_many(N, s, seeds, 60, **kw)
    t3.assert_equal(t3.merge(t3.run_cut(t3.tabu_many, N, s, seeds, (7, 1, 52), **kw)), whole, "the restatement, 7 + 1 + 52")


def test_best_state_is_a_single_queen_minimum():
    """Consequence (c): where an iteration ran behind best_iter, mcq_quench3d moves nothing on best_state."""
    checked = 0
    for idx, (N, Q, n, iters, kw) in enumerate(((4, None, 8, 60, dict(tenure=3)), (6, None, 6, 200, dict(tenure=5, tenure_rand=3)),
                                                (8, 40, 4, 200, dict(tenure=8, tenure_conf=4)), (13, None, 2, 400, dict(tenure=6)), (20, 60, 1, 200, dict(tenure=4)))):
        s = q3.random_placements(N, n, 600 + idx, Q=Q, over=idx % 2 == 0)
        got = quench.tabu_queens_host(N, s, abi.seeds_for(30 + idx, n), iters, Q=Q, hist=True, **kw)
        hist = got["energy_hist"].astype(np.int64)
        np.testing.assert_array_equal(got["best_energy"], hist.min(axis=1))
        np.testing.assert_array_equal(got["best_iter"], hist.argmin(axis=1))  # the first of the smallest
        np.testing.assert_array_equal(got["energy_in"], hist[:, 0])
        np.testing.assert_array_equal(got["energy_out"], hist[:, -1])
        assert ((got["n_moves"] + got["n_stalled"]) == iters).all() and (got["n_uphill"] <= got["n_moves"]).all() and (got["n_aspired"] <= got["n_moves"]).all()
        for r in range(n):
            assert q3.pairwise_energy(N, got["state"][r]) == int(got["energy_out"][r])
            assert q3.pairwise_energy(N, got["best_state"][r]) == int(got["best_energy"][r])
        applies = got["best_iter"] < iters
        q = quench.quench_queens_host(N, got["best_state"], Q=Q)
        assert not q["n_moves"][applies].any(), f"N={N}: a single queen's move lowers best_state"
        checked += int(applies.sum())
    assert checked >= 12


def test_a_repeated_placement_among_sound_ones():
    for N, Q in ((4, None), (13, 30), (20, None)):
        n, iters = 4, 5
        s = q3.random_placements(N, n, 20 + N, Q=Q, over=True)
        s[2, 3:6] = s[2, 0:3]  # queen 1 onto queen 0
        seeds = abi.seeds_for(8, n)
        tin = np.random.RandomState(N).randint(0, 9, size=(n, N ** 3)).astype(np.uint16)
        got = quench.tabu_queens_host(N, s, seeds, iters, Q=Q, tenure=3, tabu_in=tin, best_floor=np.zeros(n, dtype=np.int32), **ALL)
        np.testing.assert_array_equal(got["flags"], [0, 0, abi.TABU3D_REPEATED, 0])
        e = q3.pairwise_energy(N, s[2])
        assert (got["energy_hist"][2] == e).all() and got["energy_in"][2] == got["energy_out"][2] == got["best_energy"][2] == e
        np.testing.assert_array_equal(got["state"][2], np.minimum(s[2], N - 1))
        np.testing.assert_array_equal(got["best_state"][2], np.minimum(s[2], N - 1))
        np.testing.assert_array_equal(got["tabu_out"][2], tin[2])
        assert not any(got[k][2] for k in t3.COUNTERS + ("best_iter",))
        assert not quench.tabu_queens_host(N, s, seeds, iters, Q=Q, tabu_out=True)["tabu_out"][2].any()
        if N == 4:
            t3.assert_equal(got, t3.tabu_many(N, s, seeds, iters, Q=Q, tenure=3, tabu_in=tin, best_floor=np.zeros(n, dtype=np.int64)), "a repeat among sound placements")


def test_first_iter_on_both_sides_of_2_32():
    """The counter's second word goes from 0 to 1 inside the run."""
    for N, Q, n, first in ((4, None, 3, (1 << 32) - 30), (5, 30, 2, (1 << 32) - 1), (5, None, 2, (1 << 32)), (6, None, 1, (1 << 33) - 20)):
        s, seeds = q3.random_placements(N, n, 70 + N, Q=Q, over=True), abi.seeds_for(11 + N, n)
        kw = dict(Q=Q, tenure=3, tenure_rand=5, tenure_conf=4, first_iter=first)
        want = t3.tabu_many(N, s, seeds, 60, **kw)
        t3.assert_equal(quench.tabu_queens_host(N, s, seeds, 60, **ALL, **kw), want, f"N={N} first_iter={first}")
        t3.assert_equal(t3.merge(t3.run_cut(quench.tabu_queens_host, N, s, seeds, (7, 1, 52), **ALL, **kw)), want, f"N={N} first_iter={first}: cut")
    g = (1 << 32) + 6  # the restated draw past the mark takes the high counter word: it is not the draw of a counter that dropped it
    x = t3.philox((6, 1, 0, 0), (11, 8))
    assert t3.draw(11, g, 5, 25, 9) == ((x[0] * 25) >> 32, (x[1] * 10) >> 32, (x[2] * 125) >> 32) and x != t3.philox((6, 0, 0, 0), (11, 8))
    assert t3.philox((0, 0, 0, 0), (0, 0)) == (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)  # the known answer of philox4x32-10
    a = quench.tabu_queens_host(4, q3.random_placements(4, 2, 5), abi.seeds_for(3, 2), 40, tenure=2, first_iter=6, hist=True)
    b = quench.tabu_queens_host(4, q3.random_placements(4, 2, 5), abi.seeds_for(3, 2), 40, tenure=2, first_iter=g, hist=True)
    assert not np.array_equal(a["energy_hist"], b["energy_hist"])


def test_in_place_and_optional_outputs():
    N, n = 5, 5
    s, seeds = q3.random_placements(N, n, 3, over=True), abi.seeds_for(8, n)
    tin = np.random.RandomState(1).randint(0, 9, size=(n, N ** 3)).astype(np.uint16)
    got = quench.tabu_queens_host(N, s, seeds, 90, tenure=4, tenure_rand=2, tabu_in=tin, tabu_out=True)
    buf, stamps = s.copy(), tin.copy()
    q = abi.Tabu3d()
    q.N, q.n_queens, q.n_chains, q.n_iters, q.tenure, q.tenure_rand = N, 0, n, 90, 4, 2
    q.seeds, q.state_in, q.state_out, q.tabu_in, q.tabu_out = seeds.ctypes.data, buf.ctypes.data, buf.ctypes.data, stamps.ctypes.data, stamps.ctypes.data
    mcq_amd._lib.tabu3d_host(q)
    np.testing.assert_array_equal(buf, got["state"])
    np.testing.assert_array_equal(stamps, got["tabu_out"])


def test_refusals_name_the_field():
    L = mcq_amd._lib.lib()
    buf, other = np.zeros((4, 108), dtype=np.uint8), np.zeros((4, 108), dtype=np.uint8)
    seeds = abi.seeds_for(1, 4)
    hist = np.zeros((4, 8), dtype=np.int32)

    def block(**kw):
        q = abi.Tabu3d()
        q.N, q.n_queens, q.n_chains, q.n_iters, q.first_iter, q.tenure, q.tenure_rand, q.tenure_conf = 6, 0, 4, 3, 0, 5, 0, 0
        q.seeds, q.state_in, q.state_out = seeds.ctypes.data, buf.ctypes.data, buf.ctypes.data
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    refused = ((dict(N=1), b"N out of range"), (dict(N=33), b"tabu search stops at N = 32"), (dict(N=65), b"N out of range"),
               (dict(n_queens=1), b"n_queens out of range"), (dict(n_queens=216), b"n_queens out of range"), (dict(n_queens=-3), b"n_queens out of range"),
               (dict(n_chains=0), b"n_chains"), (dict(n_chains=-1), b"n_chains"), (dict(n_chains=1 << 31), b"n_chains"),
               (dict(n_iters=-1), b"n_iters"), (dict(first_iter=-1), b"first_iter"), (dict(tenure=-1), b"tenure out of range"),
               (dict(tenure=8193), b"tenure out of range"), (dict(tenure_rand=-1), b"tenure_rand out of range"), (dict(tenure_rand=4096), b"tenure_rand out of range"),
               (dict(tenure_conf=-1), b"tenure_conf out of range"), (dict(tenure_conf=65), b"tenure_conf out of range"),
               (dict(seeds=None), b"seeds"), (dict(state_in=None), b"state_in"), (dict(state_out=None), b"state_out"),
               (dict(energy_hist=hist.ctypes.data, hist_stride=3), b"hist_stride"), (dict(energy_hist=hist.ctypes.data, hist_stride=0), b"hist_stride"),
               (dict(best_state=buf.ctypes.data), b"best_state"), (dict(state_out=other.ctypes.data, best_state=other.ctypes.data), b"best_state"),
               (dict(state_out=other.ctypes.data, best_state=buf.ctypes.data), b"best_state"),
               (dict(n_iters=1, first_iter=(1 << 63) - 1), b"2^63"), (dict(n_iters=(1 << 62), first_iter=(1 << 62)), b"2^63"))
    before = L.mcq_tabu_last_error()
    for kw, msg in refused:
        for fn in (L.mcq_tabu3d_host, lambda q: L.mcq_tabu3d_device(q, None)):  # refused before any launch: no GPU here
            assert fn(ctypes.byref(block(**kw))) == abi.EINVAL, kw
            assert msg in L.mcq_tabu3d_last_error(), (kw, L.mcq_tabu3d_last_error())
    assert L.mcq_tabu_last_error() == before  # the message is the call's own
    assert L.mcq_tabu3d_host(None) == abi.EINVAL and L.mcq_tabu3d_device(None, None) == abi.EINVAL
    # at the bounds: accepted
    assert L.mcq_tabu3d_host(ctypes.byref(block(n_iters=0, first_iter=(1 << 63) - 1))) == abi.OK
    assert L.mcq_tabu3d_host(ctypes.byref(block(tenure=8192, tenure_rand=4095, tenure_conf=64))) == abi.OK
    assert L.mcq_tabu3d_host(ctypes.byref(block(energy_hist=hist.ctypes.data, hist_stride=4))) == abi.OK
    assert L.mcq_tabu3d_host(ctypes.byref(block(hist_stride=0))) == abi.OK  # not read without energy_hist
    assert L.mcq_tabu3d_host(ctypes.byref(block(best_state=other.ctypes.data))) == abi.OK
    with pytest.raises(ValueError, match="N out of range"):
        quench.tabu_queens_host(33, np.zeros((2, 3 * 33 * 33), dtype=np.uint8), seeds[:2], 1)
    with pytest.raises(ValueError, match="tenure out of range"):
        quench.tabu_queens_host(6, buf, seeds, 1, tenure=9000)
    with pytest.raises(ValueError, match="n_chains"):
        quench.tabu_queens_host(6, np.zeros((0, 108), dtype=np.uint8), seeds[:0], 1)
    with pytest.raises(ValueError, match="seeds"):
        quench.tabu_queens_host(6, buf, seeds[:3], 1)
    with pytest.raises(ValueError, match="tabu_in"):
        quench.tabu_queens_host(6, buf, seeds, 1, tabu_in=np.zeros((4, 36), dtype=np.uint16))
    with pytest.raises(ValueError, match="best_floor"):
        quench.tabu_queens_host(6, buf, seeds, 1, best_floor=np.zeros(3, dtype=np.int32))
    with pytest.raises(ValueError, match="final_state layout"):
        quench.tabu_queens_host(6, np.zeros((2, 107), dtype=np.uint8), seeds[:2], 1)
    # the annealing hook refuses what the walk does not run before anything is launched
    lin = {"type": "linear_annealing", "beta_start": 1.0, "beta_end": 3.0}
    for kw, msg in ((dict(mcmc_type="full_3d", tabu_iters=-1), "tabu_iters must be"), (dict(mcmc_type="full_3d", tabu_iters=3, hops=2), "not both"),
                    (dict(tabu_iters=3), "full_3d placements only"), (dict(mcmc_type="full_3d", tabu_iters=3, tabu_tenure=9000), "tabu_tenure out of range"),
                    (dict(mcmc_type="full_3d", tabu_iters=3, tabu_tenure_rand=4096), "tabu_tenure_rand out of range"),
                    (dict(mcmc_type="full_3d", tabu_iters=3, Q=14273), "bytes of LDS")):
        with pytest.raises(ValueError, match=msg):
            mcq_amd.heatbath.anneal_heatbath(32 if "Q" in kw else 6, 4, "random", lin, seeds, **kw)
    quench.check_tabu_queens(0, -7, -7, 5, 99, None, board=True)  # 0 iterations: nothing is looked at


def test_the_lds_formula_and_its_refusal():
    """bytes = 4 (32 + ceil(N^3 / 2) + ceil(N^3 / (4 or 2)) + ceil(N^3 / 32) + ceil(Q / 2)): the device entry point refuses what is above
    MCQ_MAX_TABU3D_LDS before any launch (no GPU here) and names N, Q and the bytes; the host code runs the shape."""
    L = mcq_amd._lib.lib()
    assert [abi.tabu3d_lds_bytes(N) for N in (2, 3, 12, 13, 19, 20, 32)] == [4 * (32 + 4 + 2 + 1 + 2), 4 * (32 + 14 + 7 + 1 + 5), 4 * (32 + 864 + 432 + 54 + 72),
                                                                             4 * (32 + 1099 + 550 + 69 + 85), 4 * (32 + 3430 + 1715 + 215 + 181),
                                                                             4 * (32 + 4000 + 4000 + 250 + 200), 137344]
    assert all(abi.tabu3d_lds_bytes(N) <= abi.MAX_TABU3D_LDS for N in range(2, 33))  # every Q = N^2 fits
    assert abi.tabu3d_lds_bytes(32, 14272) == abi.MAX_TABU3D_LDS == 160 * 1024 and abi.tabu3d_lds_bytes(32, 0) == abi.tabu3d_lds_bytes(32)
    assert all(abi.tabu3d_lds_bytes(N, N ** 3 - 1) <= abi.MAX_TABU3D_LDS for N in range(2, 30)) and abi.tabu3d_lds_bytes(30, 30 ** 3 - 1) > abi.MAX_TABU3D_LDS
    for N, Q, fits in ((32, 14272, True), (32, 14273, False), (31, 31 ** 3 - 1, False), (29, 29 ** 3 - 1, True)):
        s = q3.random_placements(N, 1, N, Q=Q)
        out, seeds = np.zeros_like(s), abi.seeds_for(1, 1)
        q = abi.Tabu3d()
        q.N, q.n_queens, q.n_chains, q.n_iters, q.tenure = N, Q, 1, 1, 3
        q.seeds, q.state_in, q.state_out = seeds.ctypes.data, s.ctypes.data, out.ctypes.data
        if not fits:
            assert L.mcq_tabu3d_device(ctypes.byref(q), None) == abi.EINVAL
            msg = L.mcq_tabu3d_last_error().decode()
            assert f"N = {N} with n_queens = {Q}" in msg and f"{abi.tabu3d_lds_bytes(N, Q)} bytes of LDS" in msg, msg
        assert L.mcq_tabu3d_host(ctypes.byref(q)) == abi.OK  # every shape
        assert (out != s).any()


def test_struct_layout_and_build():
    fields = [f for f, _ in abi.Tabu3d._fields_]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "mcq.h"\nint main(){printf("%zu %d %d %d %d", sizeof(mcq_tabu3d), MCQ_ABI_VERSION, ' \
        'MCQ_MAX_TABU3D_SPAN, MCQ_MAX_TABU3D_LDS, MCQ_TABU3D_REPEATED);' + \
        "".join(f'printf(" %zu", offsetof(mcq_tabu3d, {f}));' for f in fields) + "return 0;}"
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(prog)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")], check=True)
        out = subprocess.run([os.path.join(d, "t")], capture_output=True, text=True, check=True).stdout.split()
    assert int(out[0]) == ctypes.sizeof(abi.Tabu3d) and int(out[1]) == 6 == abi.ABI_VERSION
    assert [int(x) for x in out[2:5]] == [abi.MAX_TABU3D_SPAN, abi.MAX_TABU3D_LDS, abi.TABU3D_REPEATED]
    assert [int(x) for x in out[5:]] == [getattr(abi.Tabu3d, f).offset for f in fields]
    assert set(abi.TABU3D_DTYPES) | {"state", "best_state"} == set(t3.FIELDS) == set(quench.FIELDS_TABU3D) == set(quench.FIELDS_TABU) | {"flags"}
    b = mcq_amd.build
    assert b.TABU3D_SOURCES == [os.path.join(b.CSRC, "mcq_tabu3d.hip")] and os.path.exists(b.TABU3D_SOURCES[0])
    assert not set(b.TABU3D_SOURCES) & set(b.SOURCES + b.ADDED_SOURCES + b.TEMPER_SOURCES + b.TEMPER3D_SOURCES + b.PAIRS_SOURCES + b.HOP_SOURCES + b.HOP3D_SOURCES
                                           + b.TABU_SOURCES)
    L = mcq_amd._lib.lib()
    for name in ("mcq_tabu3d_device", "mcq_tabu3d_host", "mcq_tabu3d_last_error"):
        assert hasattr(L, name), name
