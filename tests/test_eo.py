"""GPU: the extremal-optimisation kernel (mcq_eo_device) against the library's host code (mcq_eo_host) bit for bit on every output,
histories included, at both ends of every instantiation with ragged chain counts, both moves, with and without the history; in place
and on a stream of its own; cut runs; first_iter across 2^32; the rank tables where a rank search goes wrong -- every entry 0, every
entry 2^32 - 1, positions on the first and on the last column of every value class, classes that wrap past the offset o --; a placement
of energy 0; the largest lambda N = 32 allows; and the distribution of the drawn rank over 16 384 chains.  tests/test_eo_host.py holds
the host code to the restatement of tests/eo_util.py; what a comparison here has to contain is asserted from the restatement's traces
or the host code's outputs, never from the kernel's."""
import functools

import numpy as np
import pytest

import mcq_amd
from tests import eo_util as eu

abi = mcq_amd.abi
eo = mcq_amd.eo
pytestmark = pytest.mark.gpu

GROUPS = {4: (2, 4), 8: (5, 8), 12: (9, 12), 16: (13, 16), 24: (17, 24), 32: (25, 32)}  # both ends of every instantiation
CHAINS = {2: 70, 4: 67, 5: 65, 8: 64, 9: 63, 12: 37, 13: 33, 16: 21, 17: 13, 24: 7, 25: 5, 32: 3}
ITERS = {2: 400, 4: 400, 5: 400, 8: 400, 9: 300, 12: 300, 13: 300, 16: 300, 17: 200, 24: 200, 25: 200, 32: 200}


def _case(N):
    n = CHAINS[N]
    return eu.random_boards(N, n, 300 + N, over=True), abi.seeds_for(77 + N, n), ITERS[N]


@pytest.mark.parametrize("NP", sorted(GROUPS))
def test_kernel_equals_the_host_code(NP):
    for N in GROUPS[NP]:
        s, seeds, iters = _case(N)
        assert int(s.max()) >= N  # clamped bytes among the inputs
        for move in eo.MOVES:
            for tau in (1.4, 0.0):
                want = eo.eo_states_host(N, s, seeds, iters, tau=tau, move=move, hist=True)
                assert (want["n_moves"] + want["n_idle"] == iters).all() and want["n_flat"].sum() > 0
                assert N == 2 or (want["n_uphill"].sum() > 0 and (want["best_iter"] > 0).any())
                got = eo.eo_states(N, s, seeds, iters, tau=tau, move=move, hist=True)
                what = f"N={N} chains={len(s)} {move} tau={tau}"
                eu.assert_equal(got, want, what)
                assert set(got) == set(eo.FIELDS)
                for k, dt in abi.EO_DTYPES.items():
                    assert got[k].dtype == dt, k
            slim = eo.eo_states(N, s, seeds, iters, tau=0.0, move=move)
            assert "energy_hist" not in slim
            eu.assert_equal(slim, want, f"N={N} {move}: without the history", fields=[k for k in eu.FIELDS if k in slim])


def test_no_iterations_is_the_recount():
    for N, n in ((5, 4), (13, 2), (32, 1)):
        s, seeds = eu.random_boards(N, n, 9 + N, over=True), abi.seeds_for(1, n)
        got = eo.eo_states(N, s, seeds, 0, first_iter=(1 << 40) + 3, hist=True)
        eu.assert_equal(got, eo.eo_states_host(N, s, seeds, 0, first_iter=(1 << 40) + 3, hist=True), f"N={N}: n_iters=0")
        np.testing.assert_array_equal(got["state"], np.minimum(s, N - 1))
        np.testing.assert_array_equal(got["best_state"], np.minimum(s, N - 1))
        floor = got["energy_in"].astype(np.int64) - np.arange(n) + 1
        np.testing.assert_array_equal(eo.eo_states(N, s, seeds, 0, best_floor=floor.astype(np.int32))["best_energy"], np.minimum(floor, got["energy_in"]))


@pytest.mark.parametrize("move", eo.MOVES)
def test_a_cut_run_is_the_unbroken_run(move):
    N, n = 12, 65
    s, seeds = eu.random_boards(N, n, 52, over=True), abi.seeds_for(9, n)
    whole = eo.eo_states_host(N, s, seeds, 400, move=move, first_iter=4, hist=True)
    assert (whole["best_iter"] > 8).any() and whole["n_uphill"].sum() > 0
    for cuts in ((7, 1, 392), (399, 1), (200, 0, 200)):
        parts = eu.run_cut(eo.eo_states, N, s, seeds, cuts, first_iter=4, move=move)
        eu.assert_equal(eu.merge(parts), whole, f"N=12 {move}: cut {cuts}")


@pytest.mark.parametrize("N,n", ((6, 9), (13, 5), (25, 3)))
def test_first_iter_across_2_32(N, n):
    s, seeds = eu.random_boards(N, n, 70 + N), abi.seeds_for(5 + N, n)
    first, iters = (1 << 32) - 5, 60
    want = eo.eo_states_host(N, s, seeds, iters, first_iter=first, hist=True)
    got = eo.eo_states(N, s, seeds, iters, first_iter=first, hist=True)
    eu.assert_equal(got, want, f"N={N} first_iter=2^32 - 5")
    parts = eu.run_cut(eo.eo_states, N, s, seeds, (5, 55), first_iter=first)
    eu.assert_equal(eu.merge(parts), want, f"N={N}: cut at 2^32")
    # a counter without its high word runs the iterations 0 .. 54 behind the first five: another run, on the device as in host code
    dropped = eo.eo_states(N, parts[0]["state"], seeds, 55, first_iter=0, best_floor=parts[0]["best_energy"], hist=True)
    eu.assert_equal(dropped, eo.eo_states_host(N, parts[0]["state"], seeds, 55, first_iter=0, best_floor=parts[0]["best_energy"], hist=True), f"N={N}: from 0")
    assert (dropped["energy_hist"] != got["energy_hist"][:, 5:]).any(axis=1).all()


def _one_placement(N, n, seed):
    """n chains on one random placement: the seeds alone tell them apart."""
    return np.repeat(eu.random_boards(N, 1, seed), n, axis=0), abi.seeds_for(seed, n)


@pytest.mark.parametrize("N", (5, 12, 13, 25))
def test_the_tables_where_a_rank_search_goes_wrong(N):
    Q, n, iters = N * N, 24, 40
    s, seeds = _one_placement(N, n, 600 + N)
    lam = eu.badness(N, eu.clamp(N, s[0]))
    sizes = [int((lam == v).sum()) for v in sorted(set(lam.tolist()), reverse=True)]  # the value classes, the worst first
    assert len(sizes) >= 3 and sum(sizes) == Q
    firsts = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    lasts = np.cumsum(sizes) - 1
    positions = sorted(set(firsts.tolist()) | set(lasts.tolist()))
    assert positions[0] == 0 and positions[-1] == Q - 1
    hit_first = hit_last = wraps_low = wraps_high = 0
    for j in positions:
        tab = eu.step_table(N, j)  # j entries of 0: position j in every iteration
        want = eo.eo_states_host(N, s, seeds, iters, rank_cdf=tab, hist=True)
        eu.assert_equal(eo.eo_states(N, s, seeds, iters, rank_cdf=tab, hist=True), want, f"N={N}: position {j}")
        for r in range(0, n, 6):  # the first iteration of a few chains through the restatement: where position j lies
            one = eu.eo(N, s[r], int(seeds[r]), 1, rank_cdf=tab)
            tr = one["trace"][0]
            assert tr["j"] == j and one["state"].tolist() == eo.eo_states_host(N, s[r], seeds[r: r + 1], 1, rank_cdf=tab)["state"][0].tolist()
            hit_first += tr["first_of_class"]
            hit_last += tr["last_of_class"]
            wraps_low += tr["class_wraps"] and tr["wrapped"]       # the class straddles o and the column lies below it
            wraps_high += tr["class_wraps"] and not tr["wrapped"]
    assert hit_first >= len(sizes) and hit_last >= len(sizes) and wraps_low > 0 and wraps_high > 0, (hit_first, hit_last, wraps_low, wraps_high)
    # every entry 0: j = N^2 - 1, the last column of the lowest class; every entry 2^32 - 1: j = 0 unless x0 = 2^32 - 1
    for tab in (np.zeros(Q - 1, dtype=np.uint32), np.full(Q - 1, 0xFFFFFFFF, dtype=np.uint32), np.full(1, 0xFFFFFFFF, dtype=np.uint32), np.zeros(0, dtype=np.uint32)):
        for move in eo.MOVES:
            want = eo.eo_states_host(N, s, seeds, iters, rank_cdf=tab, move=move, hist=True)
            eu.assert_equal(eo.eo_states(N, s, seeds, iters, rank_cdf=tab, move=move, hist=True), want, f"N={N}: {len(tab)} entries of {tab[:1]}, {move}")


@pytest.mark.parametrize("N", (11, 13))
def test_a_placement_of_energy_0_idles(N):
    k = eu.klarner(N)
    assert not eu.badness(N, eu.clamp(N, k)).any()
    s = np.stack([k, eu.random_boards(N, 1, 3)[0], k])
    seeds = abi.seeds_for(2, 3)
    for move in eo.MOVES:
        got = eo.eo_states(N, s, seeds, 50, move=move, hist=True)
        eu.assert_equal(got, eo.eo_states_host(N, s, seeds, 50, move=move, hist=True), f"N={N} {move}")
        assert got["n_idle"].tolist() == [50, 0, 50] and got["n_moves"].tolist() == [0, 50, 0] and not got["energy_hist"][0].any()
        np.testing.assert_array_equal(got["state"][0], k)
        np.testing.assert_array_equal(got["best_state"][2], k)


def test_the_largest_lambda_of_n_32():
    """lambda <= 4 (N - 1) = 124 is the bound of the rank search's seven bits.  No column of an even board lies on both long diagonals,
    so the largest lambda N = 32 allows is 31 + 31 + 31 + 30 = 123: column (15, 15) with every aligned column at its height."""
    N, c0 = 32, 15 * 32 + 15
    s = eu.random_boards(N, 2, 41)
    for c2, _ in eu._aligned(N, c0):
        s[0, c2] = s[0, c0]
    lam = eu.badness(N, eu.clamp(N, s[0]))
    assert lam[c0] == 123 == lam.max() and (lam == 123).sum() == 1 and len(eu._aligned(N, c0)) == 123
    seeds = abi.seeds_for(8, 2)
    for move in eo.MOVES:
        for tab in (eo.rank_table(N, np.inf), eo.rank_table(N, 1.4)):
            want = eo.eo_states_host(N, s, seeds, 60, rank_cdf=tab, move=move, hist=True)
            eu.assert_equal(eo.eo_states(N, s, seeds, 60, rank_cdf=tab, move=move, hist=True), want, f"N=32 {move}")
        # under tau = infinity the first move is that column's
        assert eu.eo(N, s[0], int(seeds[0]), 1, rank_cdf=eo.rank_table(N, np.inf), move=move)["trace"][0]["c"] == c0
    worst = eo.eo_states(N, s, seeds, 1, rank_cdf=eo.rank_table(N, np.inf), hist=True)
    assert worst["state"][0, c0] != s[0, c0] and worst["energy_hist"][0, 1] - worst["energy_hist"][0, 0] <= -100


def test_in_place_and_on_a_side_stream(monkeypatch):
    import torch

    dev = torch.device("cuda", torch.cuda.current_device())
    N, n = 9, 67
    s, seeds = eu.random_boards(N, n, 5, over=True), abi.seeds_for(6, n)
    want = eo.eo_states_host(N, s, seeds, 120, move="random", hist=True)
    t, sd = torch.from_numpy(s).to(dev), torch.from_numpy(seeds.view(np.int32)).to(dev)
    res = eo.eo_device(N, t, sd, 120, move="random", hist=True, out=t)
    torch.cuda.current_stream(dev).synchronize()
    assert res["state"] is t
    eu.assert_equal(eo.to_numpy(res), want, "out = states")
    # only the placements, in place: every per-chain output is optional
    t = torch.from_numpy(s).to(dev)
    ranks = torch.from_numpy(eo.rank_table(N, 1.4).view(np.int32)).to(dev)
    q = eo._block(N, n, 120, 0, abi.EO_MOVE_RANDOM, N * N - 1)
    q.seeds, q.rank_cdf, q.state_in, q.state_out = sd.data_ptr(), ranks.data_ptr(), t.data_ptr(), t.data_ptr()
    mcq_amd._lib.eo_device(q, torch.cuda.current_stream(dev))
    torch.cuda.current_stream(dev).synchronize()
    np.testing.assert_array_equal(t.cpu().numpy(), want["state"])
    # a stream that is not the current one, with no synchronise inside; seeds as a NumPy array, the table as a tensor
    N, n = 12, 257
    s, seeds = eu.random_boards(N, n, 77), abi.seeds_for(21, n)
    want = eo.eo_states_host(N, s, seeds, 150, tau=1.2, hist=True)
    side = torch.cuda.Stream(dev)
    t, sd = torch.from_numpy(s).to(dev), torch.from_numpy(seeds.view(np.int32)).to(dev)
    ranks = torch.from_numpy(eo.rank_table(N, 1.2).view(np.int32)).to(dev)
    torch.cuda.synchronize()
    syncs = []
    real, real_all = torch.cuda.Stream.synchronize, torch.cuda.synchronize
    monkeypatch.setattr(torch.cuda.Stream, "synchronize", lambda self: (syncs.append("stream"), real(self))[1])
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: (syncs.append("device"), real_all(*a, **k))[1])
    res = eo.eo_device(N, t, sd, 150, rank_cdf=ranks, hist=True, stream=side)
    with torch.cuda.stream(side):  # (stream=None: torch's current stream, `side`): the recount of what the call before left
        res2 = eo.eo_device(N, res["state"], seeds, 0, first_iter=150, best_floor=res["best_energy"], hist=True)
    assert syncs == [], "eo_device synchronised"
    monkeypatch.undo()
    side.synchronize()
    assert res["state"] is not t
    np.testing.assert_array_equal(t.cpu().numpy(), s)
    eu.assert_equal(eo.to_numpy(res), want, "side stream")
    got2 = eo.to_numpy(res2)
    for k in ("state", "best_energy", "energy_out"):
        np.testing.assert_array_equal(got2[k], want[k], err_msg=k)
    np.testing.assert_array_equal(got2["energy_in"], want["energy_out"])
    with pytest.raises(ValueError, match="seeds"):
        eo.eo_device(N, t, sd[:5], 1)
    with pytest.raises(ValueError, match="uint8 tensor"):
        eo.eo_device(N, t.to(torch.int32), sd, 1)
    with pytest.raises(ValueError, match="best_floor"):
        eo.eo_device(N, t, sd, 1, best_floor=res["best_iter"])
    with pytest.raises(ValueError, match="rank_cdf"):
        eo.eo_device(N, t, sd, 1, rank_cdf=ranks.to(torch.int64))
    with pytest.raises(ValueError, match="n_ranks out of range"):
        eo.eo_device(N, t, sd, 1, rank_cdf=np.zeros(N * N, dtype=np.uint32))
    with pytest.raises(ValueError, match="Unknown move"):
        eo.eo_device(N, t, sd, 1, move="worst")


DRAW_N, DRAW_CHAINS, DRAW_FIRST_SEED = 6, 16384, 0


@functools.lru_cache(maxsize=None)
def _draws():
    """One N = 6 placement, 16 384 chains of one iteration, seeds 0 .. 16 383, through the restatement: (board, seeds, column, rank)."""
    board = eu.random_boards(DRAW_N, 1, 66)[0]
    seeds = np.arange(DRAW_FIRST_SEED, DRAW_FIRST_SEED + DRAW_CHAINS, dtype=np.uint32)
    tab = eo.rank_table(DRAW_N, 1.4)
    rows = [eu.eo(DRAW_N, board, int(sd), 1, rank_cdf=tab)["trace"][0] for sd in seeds]
    return board, seeds, np.array([tr["c"] for tr in rows]), np.array([tr["j"] for tr in rows])


def test_the_drawn_rank_follows_the_table():
    """The kernel moves the restatement's column in every one of 16 384 chains, and the share of each of the first 8 ranks lies within
    5 binomial standard deviations of the table's probability.  (The restatement alone stays inside that bound for these seeds: checked
    on the CPU before the seeds were fixed.)"""
    board, seeds, cols, ranks = _draws()
    s = np.repeat(board[None, :], DRAW_CHAINS, axis=0)
    got = eo.eo_states(DRAW_N, s, seeds, 1, rank_cdf=eo.rank_table(DRAW_N, 1.4))
    changed = got["state"] != np.minimum(s, DRAW_N - 1)
    assert (changed.sum(axis=1) == 1).all() and (got["n_moves"] == 1).all()
    np.testing.assert_array_equal(changed.argmax(axis=1), cols)
    cdf = np.concatenate([[0.0], eo.rank_table(DRAW_N, 1.4).astype(np.float64) / 2.0**32])
    for j in range(8):
        p = cdf[j + 1] - cdf[j]
        share, sigma = float((ranks == j).mean()), float(np.sqrt(p * (1.0 - p) / DRAW_CHAINS))
        print(f"rank {j}: share {share:.5f}, table {p:.5f}, {abs(share - p) / sigma:.2f} sigma")
        assert abs(share - p) <= 5.0 * sigma, (j, share, p, sigma)
