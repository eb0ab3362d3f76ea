"""GPU: the tabu kernel of full_3d placements (mcq_tabu3d_device) against the library's host code (mcq_tabu3d_host) bit for bit on every
output at both ends of every instantiation (W = 64 to N = 12, 256 to N = 19, 1024 beyond), with ragged Q, and chain 0 of every case
against the NumPy restatement (tests/tabu3d_util.py, a brute force over all pairs) -- but for Q = N^2 and Q = 1 023 at N = 32, where the
brute force is a matrix of 32 768 x 1 024 per iteration: there the restatement follows a case of 120 queens.  Then a cut run, n_iters = 0, a
repeated placement, a chain that reaches E = 0 in mid-run, runs that sleep until the stamp base moves (once per shape, and twice), stamps
at the top of the uint16 range, the ends of the packed key, first_iter across 2^32, a side stream and the annealing hook."""
import functools

import numpy as np
import pytest

import mcq_amd
from tests import quench3d_util as q3
from tests import tabu3d_util as t3

abi = mcq_amd.abi
quench = mcq_amd.quench
pytestmark = pytest.mark.gpu

ALL = dict(hist=True, tabu_out=True)
GROUPS = {12: (2, 3, 4, 12), 19: (13, 19), 32: (20, 32)}
# N -> ((Q, chains, iterations, tenure, tenure_rand, tenure_conf, with tabu_in, chain 0 restated), ..)
CASES = {
    2: ((None, 3, 40, 1, 2, 0, True, True), (7, 2, 40, 0, 0, 0, False, True)),
    3: ((None, 3, 60, 2, 3, 4, True, True), (26, 3, 60, 3, 4, 0, True, True), (7, 2, 60, 0, 9, 10, False, True)),
    4: ((None, 3, 60, 3, 2, 0, False, True), (63, 3, 60, 3, 4, 0, True, True), (21, 2, 60, 5, 0, 16, True, True)),
    12: ((None, 3, 60, 4, 3, 0, False, True), (145, 2, 60, 8, 0, 8, True, True), (1727, 1, 6, 3, 0, 0, True, True)),
    13: ((None, 3, 40, 4, 3, 0, True, True), (171, 2, 40, 8, 0, 8, False, True), (2196, 1, 4, 3, 0, 0, True, True)),
    19: ((None, 2, 20, 5, 4, 2, True, True), (365, 1, 20, 3, 0, 0, False, True)),
    20: ((None, 2, 12, 5, 4, 2, True, True), (403, 1, 30, 3, 0, 0, False, True)),
    32: ((None, 2, 40, 6, 4, 2, True, False), (120, 1, 40, 3, 5, 16, True, True), (1023, 1, 20, 8, 0, 0, False, False)),
}


@functools.lru_cache(maxsize=None)
def _reference(N, i):
    """(placements, seeds, iterations, keywords, host code's result, the restatement's result of chain 0 or None) of one comparison;
    computed once, shared and left unchanged."""
    Q, n, iters, tenure, tenure_rand, tenure_conf, with_tabu, restated = CASES[N][i]
    s = q3.random_placements(N, n, 100 * N + i, Q=Q, over=True)
    seeds = abi.seeds_for(500 + N + i, n)
    tin = np.random.RandomState(N + i).randint(0, 25, size=(n, N ** 3)).astype(np.uint16) if with_tabu else None
    kw = dict(Q=Q, tenure=tenure, tenure_rand=tenure_rand, tenure_conf=tenure_conf, tabu_in=tin)
    want = quench.tabu_queens_host(N, s, seeds, iters, **ALL, **kw)
    first = t3.tabu_many(N, s[:1], seeds[:1], iters, **dict(kw, tabu_in=None if tin is None else tin[:1])) if restated else None
    return s, seeds, iters, kw, want, first


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_kernel_equals_the_host_code(group):
    import torch

    dev = torch.device("cuda", torch.cuda.current_device())
    tally = dict()
    for N in GROUPS[group]:
        for i in range(len(CASES[N])):
            s, seeds, iters, kw, want, first = _reference(N, i)
            if first is not None:
                t3.assert_equal(t3.row(want, slice(0, 1)), first, f"N={N} case {i}: host code vs the restatement")
                for k, v in t3.tally(first["trace"]).items():
                    tally[k] = tally.get(k, 0) + v
    print(group, tally)  # the condition on the inputs, before comparing
    assert tally["moves"] >= 40 and tally["aspired"] >= 3 and tally["wrapped_q"] >= 3 and tally["wrapped_t"] >= 3 and tally["moves"] > tally["on_line"] > 0
    for N in GROUPS[group]:
        for i in range(len(CASES[N])):
            s, seeds, iters, kw, want, _ = _reference(N, i)
            what = f"N={N} case {i}: Q={kw['Q']}, {s.shape[0]} chains"
            got = quench.tabu_queens(N, s, seeds, iters, **ALL, **kw)
            t3.assert_equal(got, want, what)
            for k in quench.FIELDS_TABU3D:
                assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
            if i == 0:  # in place, and only the placements: every per-chain output is optional
                n = s.shape[0]
                t, sd = torch.from_numpy(s).to(dev), torch.from_numpy(seeds.view(np.int32)).to(dev)
                ti = None if kw["tabu_in"] is None else torch.from_numpy(kw["tabu_in"].view(np.int16)).to(dev)
                res = quench.tabu_queens_device(N, t, sd, iters, out=t, **dict(kw, tabu_in=ti))
                torch.cuda.current_stream(dev).synchronize()
                assert res["state"] is t and "energy_hist" not in res and "tabu_out" not in res
                t3.assert_equal(quench.tabu_to_numpy(res), want, what + ", in place", fields=[k for k in t3.FIELDS if k not in ("energy_hist", "tabu_out")])
                q = abi.Tabu3d()
                t2, o2 = torch.from_numpy(s).to(dev), torch.zeros_like(t)
                q.N, q.n_queens, q.n_chains, q.n_iters, q.tenure, q.tenure_rand, q.tenure_conf = N, 0, n, iters, kw["tenure"], kw["tenure_rand"], kw["tenure_conf"]
                q.seeds, q.state_in, q.state_out = sd.data_ptr(), t2.data_ptr(), o2.data_ptr()
                if ti is not None:
                    q.tabu_in = ti.data_ptr()
                mcq_amd._lib.tabu3d_device(q, torch.cuda.current_stream(dev))
                torch.cuda.current_stream(dev).synchronize()
                np.testing.assert_array_equal(o2.cpu().numpy(), want["state"])
                np.testing.assert_array_equal(t2.cpu().numpy(), s)  # out of place: the input is untouched


def test_a_cut_run_is_the_unbroken_run():
    for N, Q, n, kw in ((4, None, 5, dict(tenure=3, tenure_rand=2)), (12, None, 3, dict(tenure=6, tenure_conf=8)), (13, 100, 3, dict(tenure=5, tenure_rand=4)),
                        (20, 90, 1, dict(tenure=8192, tenure_rand=4095, tenure_conf=64))):
        s = q3.random_placements(N, n, 40 + N, Q=Q, over=True)
        seeds = abi.seeds_for(9, n)
        tin = np.random.RandomState(N).randint(0, 12, size=(n, N ** 3)).astype(np.uint16)
        whole = quench.tabu_queens(N, s, seeds, 90, Q=Q, first_iter=4, tabu_in=tin, **ALL, **kw)
        t3.assert_equal(t3.merge(t3.run_cut(quench.tabu_queens, N, s, seeds, (7, 1, 82), Q=Q, first_iter=4, tabu_in=tin, **ALL, **kw)), whole, f"N={N}: 7 + 1 + 82")
        t3.assert_equal(whole, quench.tabu_queens_host(N, s, seeds, 90, Q=Q, first_iter=4, tabu_in=tin, **ALL, **kw), f"N={N}: the unbroken run")


def test_no_iterations_is_the_recount():
    for N, Q, n in ((2, 3, 3), (12, None, 2), (13, 100, 2), (32, None, 1)):
        s = q3.random_placements(N, n, 9 + N, Q=Q, over=True)
        tin = np.random.RandomState(N).randint(0, 1 << 16, size=(n, N ** 3)).astype(np.uint16)
        seeds = abi.seeds_for(1, n)
        floor = np.array([q3.pairwise_energy(N, b) for b in s]) - np.arange(n) + 1
        got = quench.tabu_queens(N, s, seeds, 0, Q=Q, tenure=5, first_iter=(1 << 40) + 3, tabu_in=tin, best_floor=floor.astype(np.int32), **ALL)
        np.testing.assert_array_equal(got["state"], np.minimum(s, N - 1))
        np.testing.assert_array_equal(got["best_state"], np.minimum(s, N - 1))
        np.testing.assert_array_equal(got["tabu_out"], tin)
        np.testing.assert_array_equal(got["best_energy"], np.minimum(floor, floor + np.arange(n) - 1))
        t3.assert_equal(got, quench.tabu_queens_host(N, s, seeds, 0, Q=Q, tenure=5, first_iter=(1 << 40) + 3, tabu_in=tin, best_floor=floor.astype(np.int32), **ALL), f"N={N}")
        assert not quench.tabu_queens(N, s, seeds, 0, Q=Q, tabu_out=True)["tabu_out"].any()


def test_a_repeated_placement_among_sound_ones():
    for N, Q in ((4, None), (13, 30), (20, None)):
        n, iters = 4, 5
        s = q3.random_placements(N, n, 20 + N, Q=Q, over=True)
        s[2, 3:6] = s[2, 0:3]  # queen 1 onto queen 0
        seeds = abi.seeds_for(8, n)
        tin = np.random.RandomState(N).randint(0, 9, size=(n, N ** 3)).astype(np.uint16)
        for stamps in (tin, None):
            kw = dict(Q=Q, tenure=3, tabu_in=stamps, best_floor=np.zeros(n, dtype=np.int32))
            want = quench.tabu_queens_host(N, s, seeds, iters, **ALL, **kw)
            np.testing.assert_array_equal(want["flags"], [0, 0, abi.TABU3D_REPEATED, 0])
            t3.assert_equal(quench.tabu_queens(N, s, seeds, iters, **ALL, **kw), want, f"N={N}: a repeat among sound placements")


def test_a_chain_that_reaches_zero_in_mid_run():
    """Few queens at N = 4: E = 0 within a few moves, and every iteration behind it stalls, through the barriers of a stalled iteration."""
    N, n, iters = 4, 6, 50
    for Q in (3, 5):
        s = q3.random_placements(N, n, 300 + Q, Q=Q, over=True)
        s[:, 3:6] = s[:, 0:3]
        s[:, 5] = (np.minimum(s[:, 2], N - 1) + 1) % N  # queen 1 next to queen 0: every chain starts above 0
        seeds = abi.seeds_for(3, n)
        want = t3.tabu_many(N, s, seeds, iters, Q=Q, tenure=4, tenure_rand=2)
        assert (want["energy_in"] > 0).all() and (want["energy_out"] == 0).all() and (want["n_moves"] > 0).all() and (want["n_stalled"] > iters // 2).all()
        t3.assert_equal(quench.tabu_queens(N, s, seeds, iters, Q=Q, tenure=4, tenure_rand=2, **ALL), want, f"Q={Q}")


# the sleeping runs: every cell stamped 2^15 -3 .. +3, best_floor = 0, the longest tenure
SLEEP_W = t3.REBASE - 3
SLEEP_Q = {5: None, 13: 40, 20: 60}


@functools.lru_cache(maxsize=None)
def _sleeper(N, top):
    Q = SLEEP_Q[N]
    s = q3.random_placements(N, 1, 60 + N, Q=Q, over=True)
    tin = t3.sleeping(N, 1, N, t3.REBASE - 3, t3.REBASE + 4)
    if top:  # cells that stay shut for the whole call, at the top of the range and on both sides of the base's bit
        tin[0, [1, 7, 20, 33, 46]] = (65535, 65534, 65535 - 17, 32768 + 200, 32768 + 201)
    return s, abi.seeds_for(70 + N, 1), tin, Q


@pytest.mark.parametrize("N", sorted(SLEEP_Q))
def test_a_run_wakes_as_the_stamp_base_moves(N):
    """One call of 2^15 + 40 iterations: nothing moves before iteration 2^15 - 3, and from there on the run is the restated window, whose
    stamps the kernel holds relative to a base that has just moved (and writes, just before, as the largest stamps there are)."""
    s, seeds, tin, Q = _sleeper(N, N == 5)
    iters = t3.REBASE + 40
    kw = dict(Q=Q, tabu_in=tin, best_floor=np.zeros(1, dtype=np.int32), **t3.LONGEST)
    want = t3.wake(N, s, seeds, iters, tin, SLEEP_W, Q=Q, **t3.LONGEST)
    moved = [tr["moved"] for tr in want["trace"][0]]
    assert sum(moved[:3]) >= 1 and sum(moved[3:]) >= 10, "the window must move on both sides of the mark"
    got = quench.tabu_queens(N, s, seeds, iters, **ALL, **kw)
    t3.assert_asleep(got, SLEEP_W, f"N={N}")
    t3.assert_equal(got, want, f"N={N}: the kernel vs the restated window")
    t3.assert_equal(got, quench.tabu_queens_host(N, s, seeds, iters, **ALL, **kw), f"N={N}: the kernel vs host code")
    assert int(got["tabu_out"].max()) > 8192  # stamps of the longest tenure alive at the end
    if N == 5:
        assert int(got["tabu_out"].max()) == 65535 - iters  # the top of the range, through the base's move (no stamp of the run is as late)
        for n_iters in (t3.REBASE, t3.REBASE + 1, 10):  # calls that end at the mark, one behind it, and far before it
            t3.assert_equal(quench.tabu_queens(N, s, seeds, n_iters, **ALL, **kw), quench.tabu_queens_host(N, s, seeds, n_iters, **ALL, **kw), f"{n_iters} iterations")
        assert int(quench.tabu_queens(N, s, seeds, 10, **ALL, **kw)["tabu_out"].max()) == 65525


def test_a_run_that_moves_the_base_twice():
    N = 5
    s, seeds, tin, Q = _sleeper(N, True)
    iters = 2 * t3.REBASE + 300
    kw = dict(Q=Q, tabu_in=tin, best_floor=np.zeros(1, dtype=np.int32), tenure=8192, tenure_rand=4095, tenure_conf=0)
    got = quench.tabu_queens(N, s, seeds, iters, **ALL, **kw)
    t3.assert_equal(got, quench.tabu_queens_host(N, s, seeds, iters, **ALL, **kw), "2^16 + 300 iterations")
    window = t3.wake(N, s, seeds, SLEEP_W + 60, tin, SLEEP_W, Q=Q, tenure=8192, tenure_rand=4095, tenure_conf=0)
    np.testing.assert_array_equal(got["energy_hist"][:, : SLEEP_W + 61], window["energy_hist"])
    hist = got["energy_hist"][0].astype(np.int64)
    assert (np.diff(hist[2 * t3.REBASE:]) != 0).any() and (np.diff(hist[t3.REBASE + 100: 2 * t3.REBASE]) != 0).any()  # it walks on both sides of the second move
    # the cut at the second mark carries tabu_out over what the unbroken call holds across its base's second move
    parts = t3.run_cut(quench.tabu_queens, N, s, seeds, (2 * t3.REBASE, 300), Q=Q, tabu_in=tin, best_floor=np.zeros(1, dtype=np.int32), tenure=8192, tenure_rand=4095,
                       **ALL)
    t3.assert_equal(t3.merge(parts), got, "2^16 + 300, cut at 2^16")


@pytest.mark.parametrize("N", t3.KEY_N)
def test_the_ends_of_delta_in_the_key(N):
    """The largest fall and rise of tests/test_tabu3d_host.py (there the host code equals the restatement on them): at N = 19 the byte
    field holds 235 on the star's centre, at N = 32 delta = -397 and, among the losing keys of the rise, +396."""
    for kind in ("fall", "rise"):
        s, seeds, iters, kw, want = t3.key_case(N, kind)
        t3.assert_equal(quench.tabu_queens(N, s, seeds, iters, **ALL, **kw), want, f"N={N} {kind}")


def test_the_ends_of_rho_in_the_key():
    for N in (4, 32):
        s, seeds, kw, want, _ = t3.rho_case(N)
        t3.assert_equal(quench.tabu_queens(N, s, seeds, 2, **ALL, **kw), want, f"N={N}: rho_q = Q - 1 and rho_t = N^3 - 1")
    N = 27  # rho_q >= 2^14: the cube with one free cell
    s, seeds, Q, (q, t, delta, rho_q) = t3.full_cube_case(N)
    assert rho_q >= 1 << 14 and abi.tabu3d_lds_bytes(N, Q) <= abi.MAX_TABU3D_LDS
    got = quench.tabu_queens(N, s, seeds, 2, Q=Q, tenure=3, **ALL)
    moved = np.flatnonzero((got["state"].reshape(Q, 3) != s.reshape(Q, 3)).any(axis=1))
    assert list(moved) == [q] and list(got["state"].reshape(Q, 3)[q]) == [0, 1, 3] and list(np.diff(got["energy_hist"][0])) == [delta, 0]
    t3.assert_equal(got, quench.tabu_queens_host(N, s, seeds, 2, Q=Q, tenure=3, **ALL), "N=27: the full cube")


def test_first_iter_across_2_32():
    for N, Q, n, first in ((4, None, 3, (1 << 32) - 30), (13, 60, 2, (1 << 32) - 1), (20, 50, 1, (1 << 33) - 20)):
        s, seeds = q3.random_placements(N, n, 70 + N, Q=Q, over=True), abi.seeds_for(11 + N, n)
        kw = dict(Q=Q, tenure=3, tenure_rand=5, tenure_conf=4, first_iter=first)
        want = t3.tabu_many(N, s, seeds, 40, **kw)
        t3.assert_equal(quench.tabu_queens(N, s, seeds, 40, **ALL, **kw), want, f"N={N} first_iter={first}")


def test_torch_tensors_on_a_side_stream(monkeypatch):
    """tabu_queens_device on a stream that is not the current one, with no synchronise inside."""
    import torch

    dev = torch.device("cuda", torch.cuda.current_device())
    N, n = 6, 257
    s = q3.random_placements(N, n, 77, over=True)
    seeds = abi.seeds_for(21, n)
    want = quench.tabu_queens_host(N, s, seeds, 30, tenure=3, tenure_rand=2, **ALL)
    side = torch.cuda.Stream(dev)
    t, sd = torch.from_numpy(s).to(dev), torch.from_numpy(seeds.view(np.int32)).to(dev)
    torch.cuda.synchronize()
    syncs = []
    real, real_all = torch.cuda.Stream.synchronize, torch.cuda.synchronize
    monkeypatch.setattr(torch.cuda.Stream, "synchronize", lambda self: (syncs.append("stream"), real(self))[1])
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: (syncs.append("device"), real_all(*a, **k))[1])
    res = quench.tabu_queens_device(N, t.reshape(n, N * N, 3), sd, 30, tenure=3, tenure_rand=2, stream=side, **ALL)
    with torch.cuda.stream(side):  # (stream=None: torch's current stream, `side`): the run goes on from the tensors of the first call
        res2 = quench.tabu_queens_device(N, res["state"], sd, 10, tenure=3, tenure_rand=2, first_iter=30, tabu_in=res["tabu_out"], best_floor=res["best_energy"], **ALL)
    assert syncs == [], "tabu_queens_device synchronised"
    monkeypatch.undo()
    side.synchronize()
    assert tuple(res["state"].shape) == (n, N * N, 3)
    t3.assert_equal(quench.tabu_to_numpy(res), want, "side stream")
    whole = quench.tabu_queens_host(N, s, seeds, 40, tenure=3, tenure_rand=2, **ALL)
    got2 = quench.tabu_to_numpy(res2)
    for k in ("state", "energy_out", "best_energy", "tabu_out"):
        np.testing.assert_array_equal(got2[k].reshape(whole[k].shape), whole[k], err_msg=k)
    with pytest.raises(ValueError, match="seeds"):
        quench.tabu_queens_device(N, t, sd[:5], 1)
    with pytest.raises(ValueError, match="uint8 tensor"):
        quench.tabu_queens_device(N, t.to(torch.int32), sd, 1)
    with pytest.raises(ValueError, match="tabu_in"):
        quench.tabu_queens_device(N, t, sd, 1, tabu_in=torch.zeros((n, 36), dtype=torch.int16, device=dev))
    with pytest.raises(ValueError, match="bytes of LDS"):
        quench.tabu_queens_device(32, torch.zeros((1, 3 * 14273), dtype=torch.uint8, device=dev), sd[:1], 1, Q=14273)
    # the NumPy wrapper runs such a shape in host code
    big = q3.random_placements(32, 1, 3, Q=14273)
    t3.assert_equal(quench.tabu_queens(32, big, seeds[:1], 2, Q=14273, **ALL), quench.tabu_queens_host(32, big, seeds[:1], 2, Q=14273, **ALL), "above the LDS")


def test_the_annealing_hook_equals_the_composed_calls():
    heatbath = mcq_amd.heatbath
    N, n, lin = 6, 64, {"type": "linear_annealing", "beta_start": 1.0, "beta_end": 3.0}
    seeds = abi.seeds_for(42, n)
    base = heatbath.anneal_heatbath(N, 12, "random", lin, seeds, mcmc_type="full_3d")
    assert not any(k.startswith("tabu") for k in base)  # tabu_iters=0: what it was
    res = heatbath.anneal_heatbath(N, 12, "random", lin, seeds, mcmc_type="full_3d", tabu_iters=200, tabu_tenure=4, tabu_tenure_rand=3)
    for k in base:
        np.testing.assert_array_equal(res[k], base[k], err_msg=k)
    w = quench.tabu_queens(N, base["best_state"], seeds, 200, tenure=4, tenure_rand=3)
    for k, f in (("tabu_state", "best_state"), ("tabu_energy", "best_energy"), ("tabu_best_iter", "best_iter"), ("tabu_moves", "n_moves")):
        np.testing.assert_array_equal(res[k], w[f], err_msg=k)
    assert (res["tabu_energy"] <= base["best_energy"]).all() and (res["tabu_energy"] < base["best_energy"]).any()
    for r in (0, n - 1):
        assert q3.pairwise_energy(N, res["tabu_state"][r]) == int(res["tabu_energy"][r])
    # behind the quench: the walk takes the quenched placements
    both = heatbath.anneal_heatbath(N, 12, "random", lin, seeds, mcmc_type="full_3d", quench=True, tabu_iters=50)
    w2 = quench.tabu_queens(N, both["quenched_state"], seeds, 50, tenure=10)
    np.testing.assert_array_equal(both["tabu_state"], w2["best_state"])
    np.testing.assert_array_equal(both["tabu_energy"], w2["best_energy"])
    assert (w2["energy_in"] == both["quenched_energy"]).all()


def test_the_largest_shape_the_lds_admits():
    """N = 32 with Q = 14 272: a chain of exactly MCQ_MAX_TABU3D_LDS bytes, the whole LDS of a compute unit, launched; two iterations,
    the kernel against the host code (every queen conflicts in a cube that full, so F = Q and both passes run at their widest)."""
    N, Q = 32, 14272
    assert abi.tabu3d_lds_bytes(N, Q) == abi.MAX_TABU3D_LDS
    s, seeds = q3.random_placements(N, 1, 4, Q=Q, over=True), abi.seeds_for(6, 1)
    tin = np.random.RandomState(2).randint(0, 4, size=(1, N ** 3)).astype(np.uint16)
    kw = dict(Q=Q, tenure=3, tenure_rand=2, tenure_conf=64, tabu_in=tin)
    want = quench.tabu_queens_host(N, s, seeds, 2, **ALL, **kw)
    assert want["n_moves"][0] == 2 and int(want["tabu_out"].max()) == abi.MAX_TABU3D_SPAN  # (64 Q / 16 is above the cap)
    t3.assert_equal(quench.tabu_queens(N, s, seeds, 2, **ALL, **kw), want, "N=32 Q=14272")
