"""GPU: the extremal-optimisation kernel of full_3d placements (mcq_eo3d_device) against the library's host code (mcq_eo3d_host) bit for
bit on every output, histories included, at both ends of every instantiation (N = 2, 12 | 13, 19 | 20, 32) with Q = N^2 and a ragged Q,
both moves, with and without the history; no iteration; cut runs; first_iter across 2^32; in place, on a stream of its own and with
the table as a tensor; the rank tables where a rank search goes wrong; the cubes with one and with two free cells; the near-full cubes
at the last byte field and at the first 16-bit field with the largest lambda each admits; the largest LDS shape, N = 32 with Q = 32 767;
an idle and a REPEATED chain among moving ones; and the distribution of the drawn rank over 16 384 chains.  tests/test_eo3d_host.py
holds the host code to the restatement of tests/eo3d_util.py; what a comparison here has to contain is asserted from the restatement's
traces or the host code's outputs, never from the kernel's."""
import functools

import numpy as np
import pytest

import mcq_amd
from tests import eo3d_util as eu

abi = mcq_amd.abi
eo = mcq_amd.eo
pytestmark = pytest.mark.gpu

# both ends of every instantiation: N -> (chains, iterations, a Q that is no multiple of the workgroup's 64, 256 or 1024 lanes)
SHAPES = {2: (70, 300, 7), 12: (21, 300, 151), 13: (17, 200, 300), 19: (7, 200, 700), 20: (3, 150, 1100), 32: (2, 100, 1500)}


@pytest.mark.parametrize("N", sorted(SHAPES))
def test_kernel_equals_the_host_code(N):
    n, iters, ragged = SHAPES[N]
    uphill = better = 0
    for Q in (N * N, ragged):
        s, seeds = eu.random_queens(N, Q, n, 300 + N + Q, over=True), abi.seeds_for(77 + N, n)
        assert int(s.max()) >= N  # clamped bytes among the inputs
        for move in eo.MOVES:
            for tau in (1.4, 0.0):
                want = eo.eo_queens_host(N, s, seeds, iters, Q=Q, tau=tau, move=move, hist=True)
                assert (want["n_moves"] + want["n_idle"] == iters).all() and want["n_moves"].sum() > 0 and not want["flags"].any()
                uphill, better = uphill + int(want["n_uphill"].sum()), better + int((want["best_iter"] > 0).sum())
                got = eo.eo_queens(N, s, seeds, iters, Q=Q, tau=tau, move=move, hist=True)
                eu.assert_equal(got, want, f"N={N} Q={Q} chains={n} {move} tau={tau}")
                assert set(got) == set(eo.FIELDS_QUEENS)
                for k, dt in abi.EO3D_DTYPES.items():
                    assert got[k].dtype == dt, k
            slim = eo.eo_queens(N, s, seeds, iters, Q=Q, tau=0.0, move=move)
            assert "energy_hist" not in slim
            eu.assert_equal(slim, want, f"N={N} Q={Q} {move}: without the history", fields=[k for k in eu.FIELDS if k in slim])
    assert N == 2 or (uphill > 0 and better > 0), (uphill, better)  # (from the host code's outputs)


def test_no_iterations_is_the_recount():
    for N, Q, n in ((5, 25, 4), (13, 300, 2), (32, 1024, 1)):
        s, seeds = eu.random_queens(N, Q, n, 9 + N, over=True), abi.seeds_for(1, n)
        got = eo.eo_queens(N, s, seeds, 0, Q=Q, first_iter=(1 << 40) + 3, hist=True)
        eu.assert_equal(got, eo.eo_queens_host(N, s, seeds, 0, Q=Q, first_iter=(1 << 40) + 3, hist=True), f"N={N}: n_iters=0")
        np.testing.assert_array_equal(got["state"], np.minimum(s, N - 1))
        np.testing.assert_array_equal(got["best_state"], np.minimum(s, N - 1))
        floor = got["energy_in"].astype(np.int64) - np.arange(n) + 1  # above, at and below energy_in
        np.testing.assert_array_equal(eo.eo_queens(N, s, seeds, 0, Q=Q, best_floor=floor.astype(np.int32))["best_energy"], np.minimum(floor, got["energy_in"]))


@pytest.mark.parametrize("move", eo.MOVES)
def test_a_cut_run_is_the_unbroken_run(move):
    N, n = 12, 33
    s, seeds = eu.random_queens(N, N * N, n, 52, over=True), abi.seeds_for(9, n)
    whole = eo.eo_queens_host(N, s, seeds, 400, move=move, first_iter=4, hist=True)
    assert (whole["best_iter"] > 8).any() and whole["n_uphill"].sum() > 0
    for cuts in ((7, 1, 392), (399, 1), (200, 0, 200)):
        parts = eu.run_cut(eo.eo_queens, N, s, seeds, cuts, first_iter=4, move=move)
        eu.assert_equal(eu.merge(parts), whole, f"N=12 {move}: cut {cuts}")


@pytest.mark.parametrize("N,n", ((6, 9), (13, 5), (25, 2)))
def test_first_iter_across_2_32(N, n):
    s, seeds = eu.random_queens(N, N * N, n, 70 + N), abi.seeds_for(5 + N, n)
    first, iters = (1 << 32) - 5, 60
    want = eo.eo_queens_host(N, s, seeds, iters, first_iter=first, hist=True)
    got = eo.eo_queens(N, s, seeds, iters, first_iter=first, hist=True)
    eu.assert_equal(got, want, f"N={N} first_iter=2^32 - 5")
    parts = eu.run_cut(eo.eo_queens, N, s, seeds, (5, 55), first_iter=first)
    eu.assert_equal(eu.merge(parts), want, f"N={N}: cut at 2^32")
    # a counter without its high word runs the iterations 0 .. 54 behind the first five: another run, on the device as in host code
    dropped = eo.eo_queens(N, parts[0]["state"], seeds, 55, first_iter=0, best_floor=parts[0]["best_energy"], hist=True)
    eu.assert_equal(dropped, eo.eo_queens_host(N, parts[0]["state"], seeds, 55, first_iter=0, best_floor=parts[0]["best_energy"], hist=True), f"N={N}: from 0")
    assert (dropped["energy_hist"] != got["energy_hist"][:, 5:]).any(axis=1).all()


def _one_placement(N, Q, n, seed):
    """n chains on one random placement: the seeds alone tell them apart."""
    return np.repeat(eu.random_queens(N, Q, 1, seed), n, axis=0), abi.seeds_for(seed, n)


@pytest.mark.parametrize("N,n,iters", ((5, 24, 40), (13, 16, 40), (25, 8, 20)))
def test_the_tables_where_a_rank_search_goes_wrong(N, n, iters):
    Q = N * N
    s, seeds = _one_placement(N, Q, n, 600 + N)
    lam = eu.badness(eu.clamp(N, s[0]))
    sizes = [int((lam == v).sum()) for v in sorted(set(lam.tolist()), reverse=True)]  # the value classes, the worst first
    assert len(sizes) >= 3 and sum(sizes) == Q
    firsts = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    lasts = np.cumsum(sizes) - 1
    positions = sorted(set(firsts.tolist()) | set(lasts.tolist()))
    assert positions[0] == 0 and positions[-1] == Q - 1
    hit_first = hit_last = wraps_low = wraps_high = 0
    for j in positions:
        tab = eu.step_table(j)  # j entries of 0: position j in every iteration
        want = eo.eo_queens_host(N, s, seeds, iters, rank_cdf=tab, hist=True)
        eu.assert_equal(eo.eo_queens(N, s, seeds, iters, rank_cdf=tab, hist=True), want, f"N={N}: position {j}")
        first = eo.eo_queens_host(N, s, seeds, 1, rank_cdf=tab, move="random")
        for r in range(0, n, n // 4):  # the first iteration of a few chains through the restatement: where position j lies
            one = eu.eo3d(N, s[r], int(seeds[r]), 1, rank_cdf=tab, move="random")
            tr = one["trace"][0]
            assert tr["j"] == j and one["state"].tolist() == first["state"][r].tolist()
            hit_first += tr["first_of_class"]
            hit_last += tr["last_of_class"]
            wraps_low += tr["class_wraps"] and tr["wrapped"]       # the class straddles o_q and the queen lies below it
            wraps_high += tr["class_wraps"] and not tr["wrapped"]
        eu.assert_equal(eo.eo_queens(N, s, seeds, 1, rank_cdf=tab, move="random"), first, f"N={N}: position {j}, one random move",
                        fields=[k for k in eu.FIELDS if k in first])
    assert hit_first >= len(sizes) and hit_last >= len(sizes) and wraps_low > 0 and wraps_high > 0, (hit_first, hit_last, wraps_low, wraps_high)
    # every entry 0: j = Q - 1, the last queen of the lowest class; every entry 2^32 - 1: j = 0 unless x0 = 2^32 - 1
    for tab in (np.zeros(Q - 1, dtype=np.uint32), np.full(Q - 1, 0xFFFFFFFF, dtype=np.uint32), np.full(1, 0xFFFFFFFF, dtype=np.uint32), np.zeros(0, dtype=np.uint32)):
        for move in eo.MOVES:
            want = eo.eo_queens_host(N, s, seeds, iters, rank_cdf=tab, move=move, hist=True)
            eu.assert_equal(eo.eo_queens(N, s, seeds, iters, rank_cdf=tab, move=move, hist=True), want, f"N={N}: {len(tab)} entries of {tab[:1]}, {move}")


@pytest.mark.parametrize("N", (3, 5, 13, 20))
def test_the_cube_with_one_free_cell(N):
    """Q = N^3 - 1: the single free cell is the target of both moves, and the cell left is the single free cell of the next iteration.
    N^3 is no multiple of 32 at N = 3, 5 and 13, so the last occupancy dword ends in pad bits that are no free cells."""
    C = N ** 3
    Q, n, iters = C - 1, 3, 12
    holes = (0, C // 2, C - 1)
    s, seeds = np.stack([eu.cube_without(N, [h]) for h in holes]), abi.seeds_for(40 + N, n)
    for move in eo.MOVES:
        want = eo.eo_queens_host(N, s, seeds, iters, Q=Q, move=move, hist=True)
        assert (want["n_moves"] == iters).all()
        moved = want["state"].reshape(n, Q, 3) != s.reshape(n, Q, 3)
        assert moved.any()
        one = eo.eo_queens_host(N, s, seeds, 1, Q=Q, move=move)  # the first move goes into the hole
        for r, h in enumerate(holes):
            q = int(np.flatnonzero((one["state"][r] != s[r]).reshape(Q, 3).any(axis=1))[0])
            assert int(eu.cells_of(N, one["state"][r].reshape(Q, 3).astype(np.int16))[q]) == h
        eu.assert_equal(eo.eo_queens(N, s, seeds, iters, Q=Q, move=move, hist=True), want, f"N={N} {move}: one free cell")
        eu.assert_equal(eo.eo_queens(N, s, seeds, 1, Q=Q, move=move), one, f"N={N} {move}: the first move", fields=[k for k in eu.FIELDS if k in one])


@pytest.mark.parametrize("N", (3, 5, 13, 20))
def test_the_cube_with_two_free_cells(N):
    """Q = N^3 - 2 with the free cells in the first and in the last occupancy dword."""
    C = N ** 3
    Q, n, iters = C - 2, 4, 30
    s = np.stack([eu.cube_without(N, pair) for pair in ((0, C - 1), (3, C - 2), (0, 1), (C - 2, C - 1))])
    seeds = abi.seeds_for(50 + N, n)
    for move in eo.MOVES:
        want = eo.eo_queens_host(N, s, seeds, iters, Q=Q, move=move, tau=0.0, hist=True)
        assert (want["n_moves"] == iters).all()
        eu.assert_equal(eo.eo_queens(N, s, seeds, iters, Q=Q, move=move, tau=0.0, hist=True), want, f"N={N} {move}: two free cells")


@pytest.mark.parametrize("N", (19, 20))
def test_the_near_full_cube_at_the_edge_of_the_field_widths(N):
    """N = 19 is the last byte field, N = 20 the first of 16 bits.  With every cell but one taken the centre queen of N = 19 is attacked
    along all of its 13 lines, lambda = 13 (N - 1) = 234 and S = 235; an even cube has no centre, and the restatement counts 241 of the
    247 there.  The largest class holds hundreds of queens (575 at N = 19)."""
    C = N ** 3
    Q = C - 1
    s, seeds = eu.cube_without(N, [5])[None], abi.seeds_for(60 + N, 1)
    lam = eu.badness(eu.clamp(N, s[0]))
    top = int(lam.max())
    assert top == {19: 234, 20: 241}[N] <= 13 * (N - 1), top
    assert max(int((lam == v).sum()) for v in set(lam.tolist())) > 500
    for move in eo.MOVES:
        for tab in (np.zeros(0, dtype=np.uint32), eo.rank_table(N, 1.4, Q)):
            want = eo.eo_queens_host(N, s, seeds, 8, Q=Q, rank_cdf=tab, move=move, hist=True)
            eu.assert_equal(eo.eo_queens(N, s, seeds, 8, Q=Q, rank_cdf=tab, move=move, hist=True), want, f"N={N} {move}, {len(tab)} ranks")
    # without a table the first move is that of a queen of the largest lambda
    first = eo.eo_queens_host(N, s, seeds, 1, Q=Q, rank_cdf=np.zeros(0, dtype=np.uint32))
    q = int(np.flatnonzero((first["state"][0] != s[0]).reshape(Q, 3).any(axis=1))[0])
    assert lam[q] == top


def test_the_largest_shape():
    """N = 32 with Q = 32 767: 137 088 bytes of LDS, the most a chain takes.  One chain, a few iterations."""
    N = 32
    Q = N ** 3 - 1
    assert abi.eo3d_lds_bytes(N, Q) == 137088 <= abi.MAX_EO3D_LDS
    s, seeds = eu.cube_without(N, [12345])[None], abi.seeds_for(3, 1)
    for move in eo.MOVES:
        want = eo.eo_queens_host(N, s, seeds, 4, Q=Q, move=move, hist=True)
        assert want["n_moves"][0] == 4 and want["energy_in"][0] > 1 << 20
        eu.assert_equal(eo.eo_queens(N, s, seeds, 4, Q=Q, move=move, hist=True), want, f"N=32 Q={Q} {move}")
    # and with room to move: Q = 30 000
    s, seeds = eu.random_queens(N, 30000, 1, 4), abi.seeds_for(4, 1)
    want = eo.eo_queens_host(N, s, seeds, 6, Q=30000, hist=True)
    assert want["n_moves"][0] == 6
    eu.assert_equal(eo.eo_queens(N, s, seeds, 6, Q=30000, hist=True), want, "N=32 Q=30000")


@pytest.mark.parametrize("N", (5, 13, 20))
def test_an_idle_and_a_repeated_chain_among_moving_ones(N):
    """N queens: chains 0, 2 and 4 start with all of them on one line, chain 1 with none attacking another, chain 3 with two in a cell."""
    Q, n, iters = N, 5, 40
    s = eu.random_queens(N, Q, n, 80 + N)
    for r in (0, 2, 4):
        s[r] = np.stack([np.arange(Q), np.zeros(Q, dtype=np.int64), np.zeros(Q, dtype=np.int64)], axis=1).astype(np.uint8).reshape(-1)
    s[1] = eu.calm_queens(N, Q, 7)
    assert not eu.badness(eu.clamp(N, s[1])).any()
    s[3, 3:6] = s[3, 0:3]
    seeds = abi.seeds_for(2, n)
    for move in eo.MOVES:
        want = eo.eo_queens_host(N, s, seeds, iters, Q=Q, move=move, best_floor=np.zeros(n, dtype=np.int32), hist=True)
        assert want["flags"].tolist() == [0, 0, 0, abi.EO3D_REPEATED, 0] and not any(want[k][3] for k in eu.COUNTERS)
        assert want["n_idle"][1] == iters and want["n_moves"][1] == 0 and (want["n_moves"][[0, 2, 4]] >= Q // 2).all()
        assert (want["energy_in"][[0, 2, 4]] == Q * (Q - 1) // 2).all() and want["energy_in"][1] == 0
        got = eo.eo_queens(N, s, seeds, iters, Q=Q, move=move, best_floor=np.zeros(n, dtype=np.int32), hist=True)
        eu.assert_equal(got, want, f"N={N} Q={Q} {move}")
        np.testing.assert_array_equal(got["state"][3], s[3])
        np.testing.assert_array_equal(got["best_state"][3], s[3])


def test_in_place_and_on_a_side_stream(monkeypatch):
    import torch

    dev = torch.device("cuda", torch.cuda.current_device())
    N, Q, n = 9, 100, 67
    s, seeds = eu.random_queens(N, Q, n, 5, over=True), abi.seeds_for(6, n)
    want = eo.eo_queens_host(N, s, seeds, 120, Q=Q, move="random", hist=True)
    t, sd = torch.from_numpy(s).to(dev), torch.from_numpy(seeds.view(np.int32)).to(dev)
    res = eo.eo_queens_device(N, t, sd, 120, Q=Q, move="random", hist=True, out=t)
    torch.cuda.current_stream(dev).synchronize()
    assert res["state"] is t
    eu.assert_equal(eo.to_numpy(res), want, "out = states")
    # only the placements, in place: every per-chain output is optional
    t = torch.from_numpy(s).to(dev)
    ranks = torch.from_numpy(eo.rank_table(N, 1.4, Q).view(np.int32)).to(dev)
    q = eo._block_queens(N, Q, n, 120, 0, abi.EO3D_MOVE_RANDOM, Q - 1)
    q.seeds, q.rank_cdf, q.state_in, q.state_out = sd.data_ptr(), ranks.data_ptr(), t.data_ptr(), t.data_ptr()
    mcq_amd._lib.eo3d_device(q, torch.cuda.current_stream(dev))
    torch.cuda.current_stream(dev).synchronize()
    np.testing.assert_array_equal(t.cpu().numpy(), want["state"])
    # a stream that is not the current one, with no synchronise inside; seeds as a NumPy array, the table as a tensor; [n][Q][3]
    N, n = 13, 65
    Q = N * N
    s, seeds = eu.random_queens(N, Q, n, 77), abi.seeds_for(21, n)
    want = eo.eo_queens_host(N, s, seeds, 150, tau=1.2, hist=True)
    side = torch.cuda.Stream(dev)
    t, sd = torch.from_numpy(s.reshape(n, Q, 3)).to(dev), torch.from_numpy(seeds.view(np.int32)).to(dev)
    ranks = torch.from_numpy(eo.rank_table(N, 1.2, Q).view(np.int32)).to(dev)
    torch.cuda.synchronize()
    syncs = []
    real, real_all = torch.cuda.Stream.synchronize, torch.cuda.synchronize
    monkeypatch.setattr(torch.cuda.Stream, "synchronize", lambda self: (syncs.append("stream"), real(self))[1])
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: (syncs.append("device"), real_all(*a, **k))[1])
    res = eo.eo_queens_device(N, t, sd, 150, rank_cdf=ranks, hist=True, stream=side)
    with torch.cuda.stream(side):  # (stream=None: torch's current stream, `side`): the recount of what the call before left
        res2 = eo.eo_queens_device(N, res["state"], seeds, 0, first_iter=150, best_floor=res["best_energy"], hist=True)
    assert syncs == [], "eo_queens_device synchronised"
    monkeypatch.undo()
    side.synchronize()
    assert res["state"] is not t and tuple(res["state"].shape) == (n, Q, 3)
    np.testing.assert_array_equal(t.cpu().numpy().reshape(n, -1), s)
    got = {k: v.reshape(n, -1) if k in ("state", "best_state") else v for k, v in eo.to_numpy(res).items()}
    eu.assert_equal(got, want, "side stream")
    got2 = eo.to_numpy(res2)
    for k in ("best_energy", "energy_out"):
        np.testing.assert_array_equal(got2[k], want[k], err_msg=k)
    np.testing.assert_array_equal(got2["state"].reshape(n, -1), want["state"])
    np.testing.assert_array_equal(got2["energy_in"], want["energy_out"])
    with pytest.raises(ValueError, match="seeds"):
        eo.eo_queens_device(N, t, sd[:5], 1)
    with pytest.raises(ValueError, match="uint8 tensor"):
        eo.eo_queens_device(N, t.to(torch.int32), sd, 1)
    with pytest.raises(ValueError, match="states must be"):
        eo.eo_queens_device(N, t, sd, 1, Q=Q + 1)
    with pytest.raises(ValueError, match="best_floor"):
        eo.eo_queens_device(N, t, sd, 1, best_floor=res["best_iter"])
    with pytest.raises(ValueError, match="rank_cdf"):
        eo.eo_queens_device(N, t, sd, 1, rank_cdf=ranks.to(torch.int64))
    with pytest.raises(ValueError, match="n_ranks out of range"):
        eo.eo_queens_device(N, t, sd, 1, rank_cdf=np.zeros(Q, dtype=np.uint32))
    with pytest.raises(ValueError, match="Unknown move"):
        eo.eo_queens_device(N, t, sd, 1, move="worst")


DRAW_N, DRAW_Q, DRAW_CHAINS, DRAW_FIRST_SEED = 4, 16, 16384, 0


@functools.lru_cache(maxsize=None)
def _draws():
    """One N = 4 placement of 16 queens, 16 384 chains of one iteration, seeds 0 .. 16 383, through the restatement: (placement, seeds,
    queen, rank, cell)."""
    placement = eu.random_queens(DRAW_N, DRAW_Q, 1, 66)[0]
    seeds = np.arange(DRAW_FIRST_SEED, DRAW_FIRST_SEED + DRAW_CHAINS, dtype=np.uint32)
    tab = eo.rank_table(DRAW_N, 1.4, DRAW_Q)
    rows = [eu.eo3d(DRAW_N, placement, int(sd), 1, rank_cdf=tab, move="random")["trace"][0] for sd in seeds]
    return placement, seeds, np.array([tr["q"] for tr in rows]), np.array([tr["j"] for tr in rows]), np.array([tr["t"] for tr in rows])


def test_the_drawn_rank_follows_the_table():
    """The kernel moves the restatement's queen to the restatement's cell in every one of 16 384 chains, and the share of each of the
    first 8 ranks lies within 5 binomial standard deviations of the table's probability.  (The restatement alone stays inside that bound
    for these seeds: checked on the CPU before the seeds were fixed.)"""
    placement, seeds, queens, ranks, cells = _draws()
    s = np.repeat(placement[None, :], DRAW_CHAINS, axis=0)
    got = eo.eo_queens(DRAW_N, s, seeds, 1, rank_cdf=eo.rank_table(DRAW_N, 1.4, DRAW_Q), move="random")
    changed = (got["state"] != s).reshape(DRAW_CHAINS, DRAW_Q, 3).any(axis=2)
    assert (changed.sum(axis=1) == 1).all() and (got["n_moves"] == 1).all()
    np.testing.assert_array_equal(changed.argmax(axis=1), queens)
    where = got["state"].reshape(DRAW_CHAINS, DRAW_Q, 3)[np.arange(DRAW_CHAINS), queens].astype(np.int64)
    np.testing.assert_array_equal((where[:, 0] * DRAW_N + where[:, 1]) * DRAW_N + where[:, 2], cells)
    cdf = np.concatenate([[0.0], eo.rank_table(DRAW_N, 1.4, DRAW_Q).astype(np.float64) / 2.0**32])
    for j in range(8):
        p = cdf[j + 1] - cdf[j]
        share, sigma = float((ranks == j).mean()), float(np.sqrt(p * (1.0 - p) / DRAW_CHAINS))
        print(f"rank {j}: share {share:.5f}, table {p:.5f}, {abs(share - p) / sigma:.2f} sigma")
        assert abs(share - p) <= 5.0 * sigma, (j, share, p, sigma)
