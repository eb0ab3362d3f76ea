"""CPU-only: tabu search in host code (mcq_tabu_host) against its NumPy restatement (tests/tabu_util.py) on every output, histories and
tabu_out included; that the compared runs hold aspired and uphill moves, winners that are not the row-major first of their ties, a
wrapped rho, a stall above E = 0 and a new best behind a rise (from the restatement's traces, before a group counts); the whole runs of
the first, middle and last chain of every case that tests/test_tabu.py puts to the kernel; sleeping runs that wake at iteration 2^15
of a call (what the kernel's move of its stamp base is held by), the sleep itself restated once, and the three confusions of the stamps
next to that iteration shown to change a history; the top of the stamp range; the largest fall and rise; n_iters = 0; a run cut 7 + 1 +
rest; best_state against the quench; the two tenure terms alone; first_iter on both sides of 2^32; every refusal; the layout of the
mcq_tabu block."""
import ctypes
import functools
import os
import subprocess
import tempfile

import numpy as np
import pytest

import mcq_amd
from tests import heatbath_util as hb
from tests import quench_util as qu
from tests import tabu_cases as tc
from tests import tabu_util as tu

abi = mcq_amd.abi
quench = mcq_amd.quench
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# N -> [(chains, iterations, tenure, tenure_rand, tenure_conf, with tabu_in)]: the literals for which the restatement alone meets the
# coverage of its group (N <= 4 and N = 5 .. 8: the kernel's two smallest paddings).  tenure = 8192 at N = 2 and 3 is the stall.
SMALL = {
    2: [(4, 40, 8192, 0, 0, False), (4, 40, 1, 2, 0, True)],
    3: [(4, 60, 8192, 0, 0, False), (4, 60, 2, 3, 4, True)],
    4: [(3, 80, 3, 2, 0, False), (3, 80, 5, 0, 16, True)],
    5: [(3, 80, 3, 2, 0, False), (2, 80, 6, 4, 8, True)],
    6: [(2, 80, 4, 3, 0, False), (2, 80, 8, 0, 8, True)],
    8: [(2, 100, 5, 4, 0, False), (1, 100, 10, 0, 4, True)],
}
# N -> the iteration at which the compared 60 iterations begin, behind a prelude of the host code with tenure 8 + (0 .. 4) + 2 F / 16:
# deep enough in the walk that the window rises and then reaches a new best
LARGE = {17: 2306, 32: 2590}
LARGE_TENURE = dict(tenure=8, tenure_rand=4, tenure_conf=2)


def _group(N):
    return 4 if N <= 4 else 8 if N <= 8 else 32


@functools.lru_cache(maxsize=None)
def _small_case(N, i):
    """(boards, seeds, iterations, keywords, the restatement's result) of one comparison; computed once and shared, never changed."""
    n, iters, tenure, tenure_rand, tenure_conf, with_tabu = SMALL[N][i]
    s = qu.random_boards(N, n, 100 * N + i, over=True)
    tin = None
    if with_tabu:
        tin = np.random.RandomState(N + i).randint(0, 25, size=(n, N ** 3)).astype(np.uint16)
        tin[0] = 30
    seeds = abi.seeds_for(50 + N + i, n)
    kw = dict(tenure=tenure, tenure_rand=tenure_rand, tenure_conf=tenure_conf, tabu_in=tin)
    return s, seeds, iters, kw, tu.tabu_many(N, s, seeds, iters, **kw)


@functools.lru_cache(maxsize=None)
def _large_cases(N):
    """[(board, seeds, keywords, the restatement's result)] at N = 17 and 32, 1 chain x 60 iterations each: the window behind the
    prelude; a start with every entry tabu for 20 iterations and a floor of 0 (no aspiration: the stall); random stamps (aspiration)."""
    s = qu.random_boards(N, 1, 7 * N, over=True)
    seeds = abi.seeds_for(3 + N, 1)
    pre = quench.tabu_host(N, s, seeds, LARGE[N], tabu_out=True, **LARGE_TENURE)
    cases = [(pre["state"], seeds, dict(first_iter=LARGE[N], tabu_in=pre["tabu_out"], best_floor=pre["best_energy"], **LARGE_TENURE)),
             (s, abi.seeds_for(4 + N, 1), dict(tenure=3, tabu_in=np.full((1, N ** 3), 20, dtype=np.uint16), best_floor=np.zeros(1, dtype=np.int32))),
             (s, abi.seeds_for(5 + N, 1), dict(tenure=3, tenure_rand=5, tabu_in=np.random.RandomState(N).randint(0, 80, size=(1, N ** 3)).astype(np.uint16)))]
    return [(b, sd, kw, tu.tabu_many(N, b, sd, 60, **kw)) for b, sd, kw in cases]


@functools.lru_cache(maxsize=None)
def _coverage():
    cov = tu.Coverage()
    for N in SMALL:
        for i in range(len(SMALL[N])):
            cov.add(_group(N), _small_case(N, i)[4]["trace"])
    for N in LARGE:
        for case in _large_cases(N):
            cov.add(_group(N), case[3]["trace"])
    return cov


@pytest.mark.parametrize("group", (4, 8, 32))
def test_the_compared_runs_aspire_rise_rotate_wrap_and_stall(group):
    print(group, _coverage().check(group))


def _check_shapes(got, n, N, iters):
    assert set(got) == set(quench.FIELDS_TABU)
    assert got["state"].dtype == np.uint8 and got["best_state"].dtype == np.uint8 and int(got["state"].max()) < N
    assert got["energy_hist"].shape == (n, iters + 1) and got["tabu_out"].shape == (n, N ** 3)
    for k, dt in abi.TABU_DTYPES.items():
        assert got[k].dtype == dt and (k in ("energy_hist", "tabu_out") or got[k].shape == (n,)), k


@pytest.mark.parametrize("N", sorted(SMALL))
def test_host_code_equals_the_restatement(N):
    _coverage().check(_group(N))
    for i in range(len(SMALL[N])):
        s, seeds, iters, kw, want = _small_case(N, i)
        assert int(s.max()) >= N  # clamped bytes among the inputs
        got = quench.tabu_host(N, s, seeds, iters, hist=True, tabu_out=True, **kw)
        tu.assert_equal(got, want, f"N={N} case {i}")
        _check_shapes(got, s.shape[0], N, iters)
        slim = quench.tabu_host(N, s, seeds, 2, **kw)
        assert "energy_hist" not in slim and "tabu_out" not in slim


@pytest.mark.parametrize("N", sorted(LARGE))
def test_host_code_equals_the_restatement_at_large_n(N):
    _coverage().check(32)
    for i, (b, seeds, kw, want) in enumerate(_large_cases(N)):
        got = quench.tabu_host(N, b, seeds, 60, hist=True, tabu_out=True, **kw)
        tu.assert_equal(got, want, f"N={N} case {i}")
        _check_shapes(got, 1, N, 60)


@pytest.mark.parametrize("N", sorted(N for pair in tc.GROUPS.values() for N in pair))
def test_host_code_equals_the_restatement_on_whole_runs(N):
    """The comparisons of tests/test_tabu.py: the first, the middle and the last chain of every case, every iteration, every output.
    The kernel is compared with the restatement on chain 0 and with the host code on the others."""
    for i, (s, seeds, kw) in enumerate(tc.cases(N)):
        got = quench.tabu_host(N, s, seeds, tc.iters(N), **tc.ALL, **kw)
        for r in sorted({0, s.shape[0] // 2, s.shape[0] - 1}):
            tu.assert_equal(tc.row(got, r), tc.restated(N, i, r), f"N={N} case {i} chain {r}")


def test_a_sleeping_run_stalls_until_its_window():
    """The premise of tu.wake as a fact of the rule: the restatement through a whole sleeping run, every iteration from 0, is the run
    that tu.wake puts together from the window."""
    N, variant = 9, "edge"
    s, seeds, tin, W, want = tc.sleep_case(N, variant)
    whole = tu.tabu(N, s[0], int(seeds[0]), tc.SLEEP_ITERS, tabu_in=tin[0], best_floor=0, **tu.LONGEST)
    assert not any(tr["moved"] for tr in whole["trace"][:W]) and sum(tr["moved"] for tr in whole["trace"]) > 100
    tu.assert_equal(whole, tc.row(want, 0), f"N={N}: the whole sleeping run")
    assert [tr["moved"] for tr in whole["trace"][W:]] == [tr["moved"] for tr in want["trace"][0]]


@pytest.mark.parametrize("variant", tc.VARIANTS)
@pytest.mark.parametrize("N", sorted(tc.SLEEP_CHAINS))
def test_host_code_wakes_at_iteration_2_15(N, variant):
    """Sleeping runs of 2^15 + 332 iterations under the longest tenure, and calls of exactly 2^15 and 2^15 + 1 iterations: the host
    code (which has no stamp base) equals the restated window on every output.  What the kernel is compared with in tests/test_tabu.py."""
    print(N, variant, tc.check_wakes(N, variant))
    s, seeds, tin, W, want = tc.sleep_case(N, variant, more=True)
    kw = tc.sleep_kw(N, variant, more=True)
    assert len(s) in (2, 3)
    for n_iters in (tc.SLEEP_ITERS, tu.REBASE, tu.REBASE + 1):
        got = quench.tabu_host(N, s, seeds, n_iters, **tc.ALL, **kw)
        tu.assert_asleep(got, W, f"N={N} {variant} {n_iters}")
        tu.assert_equal(got, tc.sleep_case(N, variant, n_iters, more=True)[4], f"N={N} {variant}: {n_iters} iterations")
    assert int(tc.sleep_case(N, variant, tu.REBASE, more=True)[4]["tabu_out"].max()) > 8192  # stamps alive at the end of the call that ends at the mark
    if N <= 13:  # 2^16 iterations: the cut at 2^15 carries tabu_out over what would be a base's second move
        whole = quench.tabu_host(N, s, seeds, 2 * tu.REBASE, **tc.ALL, **kw)
        tu.assert_equal(tu.merge(tu.run_cut(quench.tabu_host, N, s, seeds, (tu.REBASE, tu.REBASE), **tc.ALL, **kw)), whole, f"N={N} {variant}: 2^15 + 2^15")
        np.testing.assert_array_equal(whole["energy_hist"][:, : tc.SLEEP_ITERS + 1], want["energy_hist"])
        assert (np.diff(whole["energy_hist"].astype(np.int64)[:, tc.SLEEP_ITERS:], axis=1) != 0).any(axis=1).all() and int(whole["tabu_out"].max()) > 0


@pytest.mark.parametrize("NP", (12, 16, 24, 32))
def test_the_stamps_next_to_the_mark_decide(NP):
    """The edge variant cut at iteration 2^15 with tabu_out carried: the stamps that a base moved by 2^15 must hold.  A stamp equal to
    2^15 reads 0 (free), 2^15 + 1 reads 1 (tabu for one more iteration), 2^15 + 2 reads 2; each of the three confusions, put into the
    carried stamps, changes a history of this group, so a kernel that commits one cannot equal the restatement."""
    changed = dict.fromkeys(("1 -> 0", "2^15: 0 -> 1", "2 -> 1"), 0)
    for N in tc.GROUPS[NP]:
        s, seeds, tin, W, want = tc.sleep_case(N, "edge")
        n, rest = len(s), 40
        head = tu.tabu_many(N, s, seeds, tu.REBASE - W, first_iter=W, tabu_in=tin.astype(np.int64) - W, best_floor=np.zeros(n, dtype=np.int64), **tu.LONGEST)
        carried = head["tabu_out"]
        assert set(np.unique(carried[carried < 3])) == {0, 1, 2} and ((carried == 0) & (tin == tu.REBASE)).any()

        def tail(stamps):
            return tu.tabu_many(N, head["state"], seeds, rest, first_iter=tu.REBASE, tabu_in=stamps, best_floor=np.zeros(n, dtype=np.int64), **tu.LONGEST)["energy_hist"]

        np.testing.assert_array_equal(tail(carried), want["energy_hist"][:, tu.REBASE : tu.REBASE + rest + 1])
        for what, stamps in (("1 -> 0", np.where(carried == 1, 0, carried)), ("2^15: 0 -> 1", np.where((carried == 0) & (tin == tu.REBASE), 1, carried)),
                             ("2 -> 1", np.where(carried == 2, 1, carried))):
            changed[what] += int((tail(stamps) != tail(carried)).any(axis=1).sum())
    print(NP, changed)
    assert all(changed.values()), f"group {NP}: {changed}"


@pytest.mark.parametrize("N", (25, 32))
def test_the_top_of_the_stamp_range(N):
    """tabu_in with 65535, 65534, 32769, 32768, 32767, 1 and 0 among stamps that expire around iteration 2^15, most columns
    conflicting, the three tenure terms at their maxima: the moves just before iteration 2^15 write the largest stamps there are."""
    top, bound = tc.top_stamp(N)
    assert top >= bound and (N != 32 or bound == (1 << 15) + (1 << 14) - 1024), (top, bound)
    s, seeds, tin, W, want = tc.top_case(N)
    assert all(int((tin == v).sum()) >= 20 for v in tc.TOP_VALUES + (0, 1)) and min(tr["F"] for tr in want["trace"][0]) > 3 * N * N // 4
    got = quench.tabu_host(N, s, seeds, tc.TOP_ITERS, tabu_in=tin, best_floor=np.zeros(1, dtype=np.int32), **tc.ALL, **tu.LONGEST)
    tu.assert_asleep(got, W, f"N={N}")
    tu.assert_equal(got, want, f"N={N}: the top of the stamp range")
    assert int(got["tabu_out"].max()) == 65535 - tc.TOP_ITERS


@pytest.mark.parametrize("N", tc.KEY_N)
def test_the_largest_fall_and_the_largest_rise(N):
    """delta = -max a(c, k) from the flat board and +(max a(c, k) - 3) back onto it: at N = 32, -123 and +120."""
    for kind in ("flat", "uphill"):
        a_max, deltas = tc.check_key(N, kind)
        print(N, kind, a_max, deltas)
        b, seeds, kw, want = tc.key_case(N, kind)
        tu.assert_equal(quench.tabu_host(N, b, seeds, tc.KEY_ITERS[kind], **tc.ALL, **kw), want, f"N={N} {kind}")
    assert N != 32 or (tc.check_key(32, "flat")[1][0], tc.check_key(32, "uphill")[1][0]) == (-123, 120)


def test_no_iterations_is_the_recount():
    for N, n in ((2, 3), (5, 4), (13, 2), (32, 1)):
        s = qu.random_boards(N, n, 9 + N, over=True)
        tin = np.random.RandomState(N).randint(0, 1 << 16, size=(n, N ** 3)).astype(np.uint16)
        seeds = abi.seeds_for(1, n)
        got = quench.tabu_host(N, s, seeds, 0, tenure=5, first_iter=(1 << 40) + 3, tabu_in=tin, hist=True, tabu_out=True)
        clamped = np.minimum(s, N - 1)
        np.testing.assert_array_equal(got["state"], clamped)
        np.testing.assert_array_equal(got["best_state"], clamped)
        np.testing.assert_array_equal(got["tabu_out"], tin)
        e = np.array([qu.energy(N, b) for b in s])
        for k in ("energy_in", "energy_out", "best_energy"):
            np.testing.assert_array_equal(got[k], e, err_msg=k)
        np.testing.assert_array_equal(got["energy_hist"], e[:, None])
        for k in tu.COUNTERS + ("best_iter",):
            assert not got[k].any(), k
        tu.assert_equal(got, tu.tabu_many(N, s, seeds, 0, tenure=5, first_iter=(1 << 40) + 3, tabu_in=tin), f"N={N}: n_iters=0")
        floor = e - np.arange(n, dtype=np.int64) + 1  # above, at and below the recount
        low = quench.tabu_host(N, s, seeds, 0, best_floor=floor.astype(np.int32))
        np.testing.assert_array_equal(low["best_energy"], np.minimum(floor, e))
        assert "tabu_out" not in low and not quench.tabu_host(N, s, seeds, 0, tabu_out=True)["tabu_out"].any()


def test_a_cut_run_is_the_unbroken_run():
    for N, n, kw in ((3, 5, dict(tenure=2, tenure_rand=3)), (5, 6, dict(tenure=4, tenure_rand=2, tenure_conf=8)), (9, 3, dict(tenure=7, tenure_conf=3)),
                     (6, 4, dict(tenure=8192, tenure_rand=4095, tenure_conf=64))):
        s = qu.random_boards(N, n, 40 + N, over=True)
        seeds = abi.seeds_for(9, n)
        tin = np.random.RandomState(N).randint(0, 12, size=(n, N ** 3)).astype(np.uint16)
        whole = quench.tabu_host(N, s, seeds, 150, first_iter=4, tabu_in=tin, hist=True, tabu_out=True, **kw)
        parts = tu.run_cut(quench.tabu_host, N, s, seeds, (7, 1, 142), first_iter=4, tabu_in=tin, hist=True, tabu_out=True, **kw)
        tu.assert_equal(tu.merge(parts), whole, f"N={N}: 7 + 1 + 142 iterations")
        assert (whole["best_iter"] > 8).any(), "no chain found its best in the later calls"
        # without the stamps, without the floor and at another first_iter the pieces are other runs
        assert not np.array_equal(quench.tabu_host(N, s, seeds, 150, first_iter=5, tabu_in=tin, hist=True, **kw)["energy_hist"], whole["energy_hist"])
    # the restatement cut the same way is the restatement unbroken: consequence (b) holds for the rule, not only for the host code
    N, n, kw = 4, 3, dict(tenure=3, tenure_rand=2, tenure_conf=16)
    s, seeds = qu.random_boards(N, n, 44, over=True), abi.seeds_for(10, n)
    whole = tu.tabu_many(N, s, seeds, 60, **kw)
    parts = tu.run_cut(tu.tabu_many, N, s, seeds, (7, 1, 52), **kw)
    tu.assert_equal(tu.merge(parts), whole, "the restatement, 7 + 1 + 52")
    tu.assert_equal(quench.tabu_host(N, s, seeds, 60, hist=True, tabu_out=True, **kw), whole, "N=4 whole")


def test_best_state_is_a_single_move_minimum():
    """Consequence (c): where an iteration ran behind best_iter, mcq_quench moves nothing on best_state."""
    checked = 0
    for idx, (N, n, iters, kw) in enumerate(((4, 8, 60, dict(tenure=3)), (7, 6, 200, dict(tenure=5, tenure_rand=3)), (12, 4, 400, dict(tenure=8, tenure_conf=4)),
                                             (13, 3, 30, dict(tenure=2)), (16, 2, 500, dict(tenure=10)), (24, 1, 40, dict(tenure=4)))):
        s = qu.random_boards(N, n, 600 + idx, over=idx % 2 == 0)
        got = quench.tabu_host(N, s, abi.seeds_for(30 + idx, n), iters, hist=True, **kw)
        hist = got["energy_hist"].astype(np.int64)
        np.testing.assert_array_equal(got["best_energy"], hist.min(axis=1))
        np.testing.assert_array_equal(got["best_iter"], hist.argmin(axis=1))  # the first of the smallest
        np.testing.assert_array_equal(got["energy_in"], hist[:, 0])
        np.testing.assert_array_equal(got["energy_out"], hist[:, -1])
        assert ((got["n_moves"] + got["n_stalled"]) == iters).all() and (got["n_uphill"] <= got["n_moves"]).all() and (got["n_aspired"] <= got["n_moves"]).all()
        for r in range(n):
            assert qu.energy(N, got["state"][r]) == int(got["energy_out"][r])
            assert qu.energy(N, got["best_state"][r]) == int(got["best_energy"][r])
        applies = got["best_iter"] < iters
        q = quench.quench_states_host(N, got["best_state"])
        assert not q["n_moves"][applies].any(), f"N={N}: a single move lowers best_state"
        checked += int(applies.sum())
        late = ~applies  # the best placement is the last one: nothing says that it is a minimum, and after 30 or 40 iterations it is none
        if iters <= 40:
            assert late.all() and q["n_moves"][late].all()
    assert checked >= 15


def test_the_tenure_terms_each_alone():
    for N, n, kw in ((4, 3, dict(tenure=0, tenure_rand=6)), (5, 2, dict(tenure=0, tenure_conf=24)), (6, 2, dict(tenure=1, tenure_conf=64)),
                     (3, 3, dict(tenure=0, tenure_rand=4095))):
        s, seeds = qu.random_boards(N, n, 80 + N), abi.seeds_for(21 + N, n)
        want = tu.tabu_many(N, s, seeds, 80, **kw)
        tu.assert_equal(quench.tabu_host(N, s, seeds, 80, hist=True, tabu_out=True, **kw), want, f"N={N} {kw}")
        moves = [tr for chain in want["trace"] for tr in chain if tr["moved"]]
        assert len({tr["L"] for tr in moves}) >= (2 if "tenure_conf" in kw else 4), "the tenure never varied"
        if "tenure_conf" in kw:
            assert all(tr["L"] == kw["tenure"] + kw["tenure_conf"] * tr["F"] // 16 for tr in moves) and len({tr["F"] for tr in moves}) >= 2
        else:
            assert all(0 <= tr["L"] <= kw["tenure_rand"] for tr in moves)
    # no tenure at all: nothing is ever tabu
    got = quench.tabu_host(5, qu.random_boards(5, 3, 1), abi.seeds_for(2, 3), 50, tenure=0, tabu_out=True)
    assert not got["n_aspired"].any() and not got["n_stalled"].any() and int(got["tabu_out"].max()) <= 1


def test_first_iter_on_both_sides_of_2_32():
    """The counter's second word goes from 0 to 1 inside the run."""
    for N, n, first in ((4, 3, (1 << 32) - 30), (6, 2, (1 << 32) - 1), (5, 2, (1 << 32)), (13, 1, (1 << 33) - 20)):
        s, seeds = qu.random_boards(N, n, 70 + N, over=True), abi.seeds_for(11 + N, n)
        kw = dict(tenure=3, tenure_rand=5, tenure_conf=4, first_iter=first)
        want = tu.tabu_many(N, s, seeds, 60, **kw)
        tu.assert_equal(quench.tabu_host(N, s, seeds, 60, hist=True, tabu_out=True, **kw), want, f"N={N} first_iter={first}")
        parts = tu.run_cut(quench.tabu_host, N, s, seeds, (7, 1, 52), hist=True, tabu_out=True, **kw)
        tu.assert_equal(tu.merge(parts), want, f"N={N} first_iter={first}: cut")
    g = (1 << 32) + 6  # the restated draw past the mark takes the high counter word: it is not the draw of a counter that dropped it
    assert tu.draw(11, g, 5, 9) == ((hb.philox((6, 1, 0, 0), (11, 7))[0] * 125) >> 32, (hb.philox((6, 1, 0, 0), (11, 7))[1] * 10) >> 32)
    assert hb.philox((6, 1, 0, 0), (11, 7)) != hb.philox((6, 0, 0, 0), (11, 7))
    a = quench.tabu_host(4, qu.random_boards(4, 2, 5), abi.seeds_for(3, 2), 40, tenure=2, first_iter=6, hist=True)
    b = quench.tabu_host(4, qu.random_boards(4, 2, 5), abi.seeds_for(3, 2), 40, tenure=2, first_iter=g, hist=True)
    assert not np.array_equal(a["energy_hist"], b["energy_hist"])


def test_in_place_and_optional_outputs():
    N, n = 7, 5
    s, seeds = qu.random_boards(N, n, 3, over=True), abi.seeds_for(8, n)
    tin = np.random.RandomState(1).randint(0, 9, size=(n, N ** 3)).astype(np.uint16)
    got = quench.tabu_host(N, s, seeds, 90, tenure=4, tenure_rand=2, tabu_in=tin, tabu_out=True)
    buf, stamps = s.copy(), tin.copy()
    q = abi.Tabu()
    q.N, q.mode, q.n_chains, q.n_iters, q.tenure, q.tenure_rand = N, abi.MODE_BOARD, n, 90, 4, 2
    q.seeds, q.state_in, q.state_out, q.tabu_in, q.tabu_out = seeds.ctypes.data, buf.ctypes.data, buf.ctypes.data, stamps.ctypes.data, stamps.ctypes.data
    mcq_amd._lib.tabu_host(q)
    np.testing.assert_array_equal(buf, got["state"])
    np.testing.assert_array_equal(stamps, got["tabu_out"])


def test_refusals_name_the_field():
    L = mcq_amd._lib.lib()
    buf, other = np.zeros((4, 36), dtype=np.uint8), np.zeros((4, 36), dtype=np.uint8)
    seeds = abi.seeds_for(1, 4)
    hist = np.zeros((4, 8), dtype=np.int32)

    def block(**kw):
        q = abi.Tabu()
        q.N, q.mode, q.n_chains, q.n_iters, q.first_iter, q.tenure, q.tenure_rand, q.tenure_conf = 6, abi.MODE_BOARD, 4, 3, 0, 5, 0, 0
        q.seeds, q.state_in, q.state_out = seeds.ctypes.data, buf.ctypes.data, buf.ctypes.data
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    refused = ((dict(mode=abi.MODE_FULL3D), b"mode"), (dict(mode=7), b"mode"), (dict(N=1), b"N out of range"), (dict(N=33), b"N out of range"),
               (dict(N=128), b"N out of range"), (dict(n_chains=0), b"n_chains"), (dict(n_chains=-1), b"n_chains"), (dict(n_chains=1 << 31), b"n_chains"),
               (dict(n_iters=-1), b"n_iters"), (dict(first_iter=-1), b"first_iter"), (dict(tenure=-1), b"tenure out of range"),
               (dict(tenure=8193), b"tenure out of range"), (dict(tenure_rand=-1), b"tenure_rand out of range"), (dict(tenure_rand=4096), b"tenure_rand out of range"),
               (dict(tenure_conf=-1), b"tenure_conf out of range"), (dict(tenure_conf=65), b"tenure_conf out of range"),
               (dict(seeds=None), b"seeds"), (dict(state_in=None), b"state_in"), (dict(state_out=None), b"state_out"),
               (dict(energy_hist=hist.ctypes.data, hist_stride=3), b"hist_stride"), (dict(energy_hist=hist.ctypes.data, hist_stride=0), b"hist_stride"),
               (dict(best_state=buf.ctypes.data), b"best_state"), (dict(state_out=other.ctypes.data, best_state=other.ctypes.data), b"best_state"),
               (dict(state_out=other.ctypes.data, best_state=buf.ctypes.data), b"best_state"),
               (dict(n_iters=1, first_iter=(1 << 63) - 1), b"2^63"),
               (dict(n_iters=(1 << 62), first_iter=(1 << 62)), b"2^63"))
    before = L.mcq_hop_last_error()
    for kw, msg in refused:
        for fn in (L.mcq_tabu_host, lambda q: L.mcq_tabu_device(q, None)):  # refused before any launch: no GPU here
            assert fn(ctypes.byref(block(**kw))) == abi.EINVAL, kw
            assert msg in L.mcq_tabu_last_error(), (kw, L.mcq_tabu_last_error())
    assert L.mcq_hop_last_error() == before  # the message is the call's own
    assert L.mcq_tabu_host(None) == abi.EINVAL and L.mcq_tabu_device(None, None) == abi.EINVAL
    # at the bounds: accepted
    assert L.mcq_tabu_host(ctypes.byref(block(n_iters=0, first_iter=(1 << 63) - 1))) == abi.OK
    assert L.mcq_tabu_host(ctypes.byref(block(tenure=8192, tenure_rand=4095, tenure_conf=64))) == abi.OK
    assert L.mcq_tabu_host(ctypes.byref(block(tenure=0))) == abi.OK
    assert L.mcq_tabu_host(ctypes.byref(block(energy_hist=hist.ctypes.data, hist_stride=4))) == abi.OK
    assert L.mcq_tabu_host(ctypes.byref(block(hist_stride=0))) == abi.OK  # not read without energy_hist
    assert L.mcq_tabu_host(ctypes.byref(block(best_state=other.ctypes.data))) == abi.OK
    assert (abi.MAX_TABU_TENURE, abi.MAX_TABU_TENURE_RAND, abi.MAX_TABU_TENURE_CONF) == (8192, 4095, 64)
    assert abi.MAX_TABU_TENURE + abi.MAX_TABU_TENURE_RAND + abi.MAX_TABU_TENURE_CONF * 32 * 32 // 16 < 1 << 14
    with pytest.raises(ValueError, match="N out of range"):
        quench.tabu_host(33, np.zeros((2, 33 * 33), dtype=np.uint8), seeds[:2], 1)
    with pytest.raises(ValueError, match="tenure out of range"):
        quench.tabu_host(6, buf, seeds, 1, tenure=9000)
    with pytest.raises(ValueError, match="n_chains"):
        quench.tabu_host(6, np.zeros((0, 36), dtype=np.uint8), seeds[:0], 1)
    with pytest.raises(ValueError, match="seeds"):
        quench.tabu_host(6, buf, seeds[:3], 1)
    with pytest.raises(ValueError, match="tabu_in"):
        quench.tabu_host(6, buf, seeds, 1, tabu_in=np.zeros((4, 36), dtype=np.uint16))
    with pytest.raises(ValueError, match="best_floor"):
        quench.tabu_host(6, buf, seeds, 1, best_floor=np.zeros(3, dtype=np.int32))
    with pytest.raises(ValueError, match="final_state layout"):
        quench.tabu_host(6, np.zeros((2, 35), dtype=np.uint8), seeds[:2], 1)
    # the competition hook refuses what tabu search does not run before anything is launched
    for kw, msg in ((dict(N=33, tabu_iters=3), "N out of range"), (dict(N=6, tabu_iters=-1), "tabu_iters must be"),
                    (dict(N=6, tabu_iters=3, tabu_tenure=-1), "tabu_tenure out of range"), (dict(N=6, tabu_iters=3, tabu_tenure=9000), "tabu_tenure out of range"),
                    (dict(N=6, tabu_iters=3, hops=2), "not both")):
        with pytest.raises(ValueError, match=msg):
            mcq_amd.drivers.run_competition(n_runs=4, n_steps=10, **kw)
    with pytest.raises(ValueError, match="boards only"):
        quench.check_tabu(3, 5, 0, 6, board=False)
    quench.check_tabu(0, -7, 5, 99, board=False)  # 0 iterations: nothing is looked at


def test_struct_layout_and_build():
    fields = [f for f, _ in abi.Tabu._fields_]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "mcq.h"\nint main(){printf("%zu %d %d %d %d %d", sizeof(mcq_tabu), MCQ_ABI_VERSION, ' \
        'MCQ_MAX_TABU_TENURE, MCQ_MAX_TABU_TENURE_RAND, MCQ_MAX_TABU_TENURE_CONF, MCQ_MAX_TABU_LDS);' + \
        "".join(f'printf(" %zu", offsetof(mcq_tabu, {f}));' for f in fields) + "return 0;}"
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(prog)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")], check=True)
        out = subprocess.run([os.path.join(d, "t")], capture_output=True, text=True, check=True).stdout.split()
    assert int(out[0]) == ctypes.sizeof(abi.Tabu) and int(out[1]) == 6 == abi.ABI_VERSION
    assert [int(x) for x in out[2:6]] == [abi.MAX_TABU_TENURE, abi.MAX_TABU_TENURE_RAND, abi.MAX_TABU_TENURE_CONF, abi.MAX_TABU_LDS]
    assert [int(x) for x in out[6:]] == [getattr(abi.Tabu, f).offset for f in fields]
    assert set(abi.TABU_DTYPES) | {"state", "best_state"} == set(tu.FIELDS) == set(quench.FIELDS_TABU)
    assert [abi.tabu_lds_bytes(N) for N in (2, 4, 5, 8, 12, 16, 17, 24, 32)] == [288, 288, 2176, 2176, 6048, 14848, 47232, 47232, 108544]
    assert abi.tabu_lds_bytes(32) <= abi.MAX_TABU_LDS
    b = mcq_amd.build
    assert b.TABU_SOURCES == [os.path.join(b.CSRC, "mcq_tabu.hip")] and os.path.exists(b.TABU_SOURCES[0])
    assert not set(b.TABU_SOURCES) & set(b.SOURCES + b.ADDED_SOURCES + b.TEMPER_SOURCES + b.TEMPER3D_SOURCES + b.PAIRS_SOURCES + b.HOP_SOURCES + b.HOP3D_SOURCES)
    L = mcq_amd._lib.lib()
    for name in ("mcq_tabu_device", "mcq_tabu_host", "mcq_tabu_last_error"):
        assert hasattr(L, name), name
