"""GPU: the relinking kernel of full_3d placements (mcq_relink3d_device) against the library's host code (mcq_relink3d_host) bit for bit on
every output and dtype at both ends of every instantiation (W = 64 to N = 12, 256 to N = 19, 1024 beyond), with ragged Q and with 3 and
70 chains, and chain 0 of every case against the NumPy restatement (tests/relink3d_util.py, a brute force over all pairs) -- but for
the walk of d0 = Q = 1 024 at N = 32, where a step of the brute force is a matrix of 10^6 pairs: the whole walk is compared with the host
code and the restatement follows it for its first 40 steps.  A group's comparisons count only behind a gate on the restatement's traces
and the host code's outputs.  Then the variants (without the optional outputs, in place, a stream of its own), both repeat flags, the
ends of the packed key, the largest shape the LDS admits, the pool against its host form, and 256 tabu minima at N = 8 through the
consequences (c) and (d), checked with the quench kernel."""
import numpy as np
import pytest

import mcq_amd
from tests import quench3d_util as q3
from tests import relink3d_cases as rc
from tests import relink3d_util as ru

abi = mcq_amd.abi
quench = mcq_amd.quench
pytestmark = pytest.mark.gpu

GROUPS = {12: (2, 3, 4, 12), 19: (13, 19), 32: (20, 32)}
# N -> ((Q, chains, few cases), ..): Q = N^2 and the ragged Q of tests/test_tabu3d.py; chain 0 of every case is restated
SHAPES = {
    2: ((None, 3, False), (7, 2, False)),
    3: ((None, 3, False), (26, 3, False), (7, 2, False)),
    4: ((None, 70, False), (63, 3, False), (21, 2, False)),
    12: ((None, 3, False), (145, 2, False), (1727, 1, False)),
    13: ((None, 70, False), (171, 2, True), (2196, 1, False)),
    19: ((None, 3, True), (365, 1, True)),
    20: ((None, 3, True), (403, 1, True), (401, 2, True)),  # (401: its disjoint case is the walk of d0 = Q restated whole)
    32: ((120, 2, True),),
}


def _assert_same(got, want, what):
    ru.assert_equal(got, want, what)
    for k in quench.FIELDS_RELINK3D:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_kernel_equals_the_host_code(group):
    import torch

    dev = torch.device("cuda", torch.cuda.current_device())
    shapes = [(N, Q, n, few) for N in GROUPS[group] for Q, n, few in SHAPES[N]]
    for N, Q, n, few in shapes:  # host code vs the restatement on chain 0, before anything is launched
        for i, (name, s, g, seeds, kw) in enumerate(rc.cases(N, Q, n, few)):
            ru.assert_equal(rc.hosted(N, Q, n, few, i), rc.restated(N, Q, n, few, i, 1), f"N={N} Q={Q} {name}: host code vs the restatement", rows=slice(0, 1))
    print(group, rc.check_tally(rc.tally(shapes, rows=1), f"group {group}"))  # the gate: from the restatement's traces and the host outputs
    for N, Q, n, few in shapes:
        for i, (name, s, g, seeds, kw) in enumerate(rc.cases(N, Q, n, few)):
            what = f"N={N} Q={Q} {name}, {n} chains"
            want = rc.hosted(N, Q, n, few, i)
            _assert_same(quench.relink_queens(N, s, g, seeds, Q=Q, hist=True, **kw), want, what)
            if i > 0:
                continue
            # in place, and only the placements: every per-chain output is optional
            t, tg, sd = torch.from_numpy(s).to(dev), torch.from_numpy(g).to(dev), torch.from_numpy(seeds.view(np.int32)).to(dev)
            res = quench.relink_queens_device(N, t, tg, sd, Q=Q, out=t, **kw)
            torch.cuda.current_stream(dev).synchronize()
            assert res["state"] is t and "energy_hist" not in res
            ru.assert_equal(quench.to_numpy(res), want, what + ", in place", fields=[k for k in ru.FIELDS if k != "energy_hist"])
            np.testing.assert_array_equal(tg.cpu().numpy(), g)  # the guides stay the caller's
            t2 = torch.from_numpy(s).to(dev)
            slim = quench.relink_queens_device(N, t2, tg, sd, Q=Q, figures=False, **kw)
            torch.cuda.current_stream(dev).synchronize()
            assert set(slim) == {"state"}
            np.testing.assert_array_equal(slim["state"].cpu().numpy(), want["state"])
            np.testing.assert_array_equal(t2.cpu().numpy(), s)  # out of place: the input is untouched


def test_the_walk_of_1024_steps_at_n_32():
    """Q = N^2 = 1 024 queens, none on a cell of the guide: d0 = Q.  The whole walk against the host code, and the restatement on the
    same pair cut behind 40 steps (m^2 is above 10^6 pairs a step there, with the lanes of 16 wavefronts on them)."""
    N, n = 32, 1  # (one chain: a walk of this length is two seconds of host code)
    far = q3.random_placements(N, n, 77, Q=2 * N * N).reshape(n, 2, -1)
    s, g, seeds = far[:, 0].copy(), far[:, 1].copy(), abi.seeds_for(32, n)
    want = quench.relink_queens_host(N, s, g, seeds, min_dist=128, hist=True)
    assert (want["distance_in"] == N * N).all() and (want["n_steps"] == N * N).all() and (want["path_best_step"] > 0).all()
    _assert_same(quench.relink_queens(N, s, g, seeds, min_dist=128, hist=True), want, "N=32, d0 = Q = 1024")
    cut = ru.relink_many(N, s[:1], g[:1], seeds[:1], max_steps=40, min_dist=8)
    assert ru.tally(cut["trace"], cut)["ties"] >= 5
    np.testing.assert_array_equal(cut["energy_hist"][0], want["energy_hist"][0, :41])  # the cut walk is the head of the whole one
    host_cut = quench.relink_queens_host(N, s, g, seeds, max_steps=40, min_dist=8, hist=True)
    ru.assert_equal(host_cut, cut, "N=32, 40 steps: host code vs the restatement", rows=slice(0, 1))
    _assert_same(quench.relink_queens(N, s, g, seeds, max_steps=40, min_dist=8, hist=True), host_cut, "N=32, 40 steps")
    # minima of the square shape, relinked with their neighbour
    m, seeds = rc.minima(N, 3, 5), abi.seeds_for(33, 2)
    want = quench.relink_queens_host(N, m[:2], m[1:], seeds, min_dist=128, hist=True)
    _assert_same(quench.relink_queens(N, m[:2], m[1:], seeds, min_dist=128, hist=True), want, "N=32, minima")


def test_both_repeat_flags_among_sound_chains():
    for N, Q in ((4, None), (13, 30), (20, None)):
        n = 5
        Qn = rc.queens_of(N, Q)
        s, g = q3.random_placements(N, n, 20 + N, Q=Q, over=True), q3.random_placements(N, n, 30 + N, Q=Q, over=True)
        s[1, 3:6] = s[1, 0:3]
        g[2, 3 * (Qn - 1):] = g[2, 0:3]
        s[3, 3:6] = s[3, 0:3]
        g[3, 3:6] = g[3, 0:3]
        seeds = abi.seeds_for(8, n)
        for kw in (dict(), dict(max_steps=2)):
            want = quench.relink_queens_host(N, s, g, seeds, Q=Q, hist=True, **kw)
            np.testing.assert_array_equal(want["flags"], [0, 1, 2, 3, 0])
            assert (want["energy_hist"][1] == q3.pairwise_energy(N, s[1])).all()
            _assert_same(quench.relink_queens(N, s, g, seeds, Q=Q, hist=True, **kw), want, f"N={N}: repeats among sound chains {kw}")


@pytest.mark.parametrize("N", sorted(rc.KEY_N))
def test_the_ends_of_delta_in_the_key(N):
    """The star of the centre (tests/tabu3d_util.star): its centre queen leaves for a cell that nothing attacks, delta = -234 at N = 19
    (the byte field holds 235 there) and -397 at N = 32; with the two placements exchanged it returns, +234 and +397."""
    a, g, Q, c = rc.key_case(N)
    for s, guide, delta in ((a, g, -rc.KEY_N[N]), (g, a, rc.KEY_N[N])):
        want = ru.relink_many(N, s, guide, rc.ONE_SEED, Q=Q, min_dist=0)
        assert int(want["distance_in"][0]) == 1 and [tr["delta"] for tr in want["trace"][0]] == [delta]
        host = quench.relink_queens_host(N, s, guide, rc.ONE_SEED, Q=Q, min_dist=0, hist=True)
        ru.assert_equal(host, want, f"N={N} delta={delta}: host code vs the restatement")
        _assert_same(quench.relink_queens(N, s, guide, rc.ONE_SEED, Q=Q, min_dist=0, hist=True), host, f"N={N} delta={delta}")


def test_the_ends_of_rho_in_the_key():
    for N in (4, 32):
        a, g, Q, (q, t) = rc.rho_case(N)
        want = ru.relink_many(N, a, g, rc.ONE_SEED, Q=Q, min_dist=0)
        tr = want["trace"][0]
        assert len(tr) == 1 and (tr[0]["q"], tr[0]["c"], tr[0]["rho_q"], tr[0]["rho_t"]) == (q, t, Q - 1, N ** 3 - 1)  # all 15 bits of rho_t at N = 32
        host = quench.relink_queens_host(N, a, g, rc.ONE_SEED, Q=Q, min_dist=0, hist=True)
        ru.assert_equal(host, want, f"N={N}: host code vs the restatement")
        _assert_same(quench.relink_queens(N, a, g, rc.ONE_SEED, Q=Q, min_dist=0, hist=True), host, f"N={N}: rho_q = Q - 1 and rho_t = N^3 - 1")
    N = 27  # rho_q >= 2^14 needs Q > 2^14: the cube with one free cell fits the LDS
    a, g, seeds, Q, (q, t, rho_q) = rc.full_cube_case(N)
    assert rho_q >= 1 << 14 and abi.relink3d_lds_bytes(N, Q) <= abi.MAX_RELINK3D_LDS
    host = quench.relink_queens_host(N, a, g, seeds, Q=Q, min_dist=0, hist=True)
    assert int(host["distance_in"][0]) == 1 and int(host["path_best_step"][0]) == 1
    assert list(host["path_best_state"].reshape(Q, 3)[q]) == [0, 1, 3]
    assert list(np.flatnonzero((host["path_best_state"].reshape(Q, 3) != a.reshape(Q, 3)).any(axis=1))) == [q]
    _assert_same(quench.relink_queens(N, a, g, seeds, Q=Q, min_dist=0, hist=True), host, "N=27: the full cube")


def test_a_stream_of_its_own(monkeypatch):
    """relink_queens_device on a stream that is not the current one, with no synchronise inside; the shape [n][Q][3]; the refusals of the wrapper."""
    import torch

    dev = torch.device("cuda", torch.cuda.current_device())
    N, n = 6, 257
    m = rc.minima(N, n + 1, 77)
    s, g, seeds = m[:n], m[1:], abi.seeds_for(21, n)
    want = quench.relink_queens_host(N, s, g, seeds, min_dist=4, walk=3, hist=True)
    side = torch.cuda.Stream(dev)
    t, tg, sd = torch.from_numpy(s).to(dev), torch.from_numpy(g).to(dev), torch.from_numpy(seeds.view(np.int32)).to(dev)
    torch.cuda.synchronize()
    syncs = []
    real, real_all = torch.cuda.Stream.synchronize, torch.cuda.synchronize
    monkeypatch.setattr(torch.cuda.Stream, "synchronize", lambda self: (syncs.append("stream"), real(self))[1])
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: (syncs.append("device"), real_all(*a, **k))[1])
    res = quench.relink_queens_device(N, t.reshape(n, N * N, 3), tg.reshape(n, N * N, 3), sd, min_dist=4, walk=3, hist=True, stream=side)
    assert syncs == [], "relink_queens_device synchronised"
    monkeypatch.undo()
    side.synchronize()
    assert tuple(res["state"].shape) == (n, N * N, 3) and tuple(res["path_best_state"].shape) == (n, N * N, 3)
    ru.assert_equal(quench.to_numpy(res), want, "side stream")
    with pytest.raises(ValueError, match="seeds"):
        quench.relink_queens_device(N, t, tg, sd[:5])
    with pytest.raises(ValueError, match="uint8 tensor"):
        quench.relink_queens_device(N, t.to(torch.int32), tg, sd)
    with pytest.raises(ValueError, match="guides"):
        quench.relink_queens_device(N, t, tg[:5], sd)
    with pytest.raises(ValueError, match="distinct from guide_in"):
        quench.relink_queens_device(N, t, tg, sd, out=tg)
    with pytest.raises(ValueError, match="bytes of LDS"):
        big = torch.zeros((1, 3 * 11249), dtype=torch.uint8, device=dev)
        quench.relink_queens_device(32, big, big.clone(), sd[:1], Q=11249)


def test_the_largest_shape_the_lds_admits():
    """N = 32 with Q = 11 248: a chain of exactly MCQ_MAX_RELINK3D_LDS bytes, the whole LDS of a compute unit, launched once; two steps
    of a walk with all Q queens moving (the placements share no cell: 1.3 10^8 pairs a step), the kernel against the host code.  The
    placement is a minimum of the quench kernel, so that the local search behind two steps is a few passes and not the fifteen that a
    random placement of this density takes in host code (a pass there is Q scans of the cube)."""
    N, Q = 32, 11248
    assert abi.relink3d_lds_bytes(N, Q) == abi.MAX_RELINK3D_LDS
    s = quench.quench_queens(N, q3.random_placements(N, 1, 4, Q=Q), Q=Q, conflicts=False)["state"]
    z = s.reshape(Q, 3).astype(np.int64)
    free = np.setdiff1d(np.arange(N ** 3), (z[:, 0] * N + z[:, 1]) * N + z[:, 2])
    cells = np.random.RandomState(5).choice(free, size=Q, replace=False)
    g, seeds = np.stack([cells // (N * N), (cells // N) % N, cells % N], axis=1).astype(np.uint8).reshape(1, -1), abi.seeds_for(6, 1)
    want = quench.relink_queens_host(N, s, g, seeds, Q=Q, max_steps=2, min_dist=1, hist=True)
    assert int(want["distance_in"][0]) == Q and int(want["n_steps"][0]) == 2 and int(want["path_best_step"][0]) in (1, 2)
    _assert_same(quench.relink_queens(N, s, g, seeds, Q=Q, max_steps=2, min_dist=1, hist=True), want, "N=32 Q=11248")


@pytest.mark.parametrize("align", (True, False))
def test_the_pool_equals_its_host_form(align):
    import torch

    dev = torch.device("cuda", torch.cuda.current_device())
    N, n, rounds = 5, 96, 3
    s, seeds = rc.minima(N, n, 9), abi.seeds_for(4, n)
    want = quench.relink_queens_pool_host(N, s, seeds, rounds, align=align, partner_seed=2)
    got = quench.relink_queens_pool(N, torch.from_numpy(s).to(dev), torch.from_numpy(seeds.view(np.int32)).to(dev), rounds, align=align, partner_seed=2)
    np.testing.assert_array_equal(got["state"].cpu().numpy(), want["state"])
    np.testing.assert_array_equal(got["energy"].cpu().numpy(), want["energy"])
    np.testing.assert_array_equal(got["n_replaced"], want["n_replaced"])
    np.testing.assert_array_equal(got["best_energy"], want["best_energy"])
    assert got["n_replaced"].dtype == np.int64 and got["best_energy"].dtype == np.int32 and want["n_replaced"].sum() > 0
    img, idx, dist = quench.nearest_queens_image(N, torch.from_numpy(s).to(dev), torch.from_numpy(np.roll(s, 1, axis=0)).to(dev))
    himg, hidx, hdist = quench.nearest_queens_image(N, s, np.roll(s, 1, axis=0))
    np.testing.assert_array_equal(img.cpu().numpy(), himg)
    np.testing.assert_array_equal(idx.cpu().numpy(), hidx)
    np.testing.assert_array_equal(dist.cpu().numpy(), hdist)


def test_tabu_minima_through_the_consequences():
    """256 placements from tabu_queens at N = 8, each relinked with its neighbour: (c) state_out is a fixed point of L and (d)
    path_best_energy is E of path_best_state with energy_out not above it, both checked with the quench kernel."""
    import torch

    dev = torch.device("cuda", torch.cuda.current_device())
    N, n = 8, 256
    seeds = abi.seeds_for(88, n + 1)
    m = quench.tabu_queens(N, q3.random_placements(N, n + 1, 8), seeds, 300, tenure=6, tenure_rand=3)["best_state"]
    t, tg, sd = torch.from_numpy(m[:n].copy()).to(dev), torch.from_numpy(m[1:].copy()).to(dev), torch.from_numpy(seeds[:n].view(np.int32).copy()).to(dev)
    res = quench.relink_queens_device(N, t, tg, sd, min_dist=N * N // 8, hist=True)
    again = quench.quench_queens_device(N, res["state"], conflicts=False)
    pstar = quench.quench_queens_device(N, res["path_best_state"], max_passes=1, conflicts=False)
    guide = quench.quench_queens_device(N, tg, max_passes=1, conflicts=False)
    torch.cuda.current_stream(dev).synchronize()
    r, again, pstar, guide = quench.to_numpy(res), quench.to_numpy(again), quench.to_numpy(pstar), quench.to_numpy(guide)
    assert (r["flags"] == 0).all() and (r["distance_in"] > 0).all() and (r["n_steps"] == r["distance_in"]).all()
    assert again["n_moves"].sum() == 0 and (again["n_passes"] == 1).all()  # (c)
    np.testing.assert_array_equal(again["energy_in"], r["energy_out"])
    np.testing.assert_array_equal(pstar["energy_in"], r["path_best_energy"])  # (d)
    assert (r["energy_out"] <= r["path_best_energy"]).all()
    rows = np.arange(n)
    np.testing.assert_array_equal(r["energy_hist"][rows, r["distance_in"]], guide["energy_in"])  # (b)
    np.testing.assert_array_equal(r["energy_hist"][rows, r["path_best_step"]], r["path_best_energy"])
    np.testing.assert_array_equal(r["energy_hist"].max(axis=1), r["path_max_energy"])
    print("below both endpoints:", int((r["energy_out"] < np.minimum(r["energy_in"], guide["energy_in"])).sum()), "of", n)
