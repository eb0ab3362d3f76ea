"""GPU: the full_3d tempering kernel (mcq_temper3d_device) against the library's host code (mcq_temper3d_host) bit for bit on every
output and every instantiation, against the restatement, device segments against the unbroken launch, a ladder of equal multipliers
against the plain full_3d heat-bath kernel, one wide launch against the quench kernel's recount and the exchange's invariants,
temper_queens_device on torch tensors on a stream of its own, and anneal_tempered(mcmc_type="full_3d") against the same run composed on
the host."""
import numpy as np
import pytest

import mcq_amd
from tests import quench3d_util as q3
from tests import temper3d_util as t3

abi = mcq_amd.abi
heatbath = mcq_amd.heatbath
quench = mcq_amd.quench
tempering = mcq_amd.tempering
pytestmark = pytest.mark.gpu

# the seven instantiations (lanes per chain, field bits, steps) at the smallest and the largest N each serves:
#   (64, 8, 32) N = 2 .. 12 with every R; (256, 8, 64) N = 13 .. 19 with R = 2, 4; (128, 8, 64) N = 13 .. 19 with R = 8;
#   (64, 8, 64) N = 13 .. 18 with R = 16; (512, 16, 64) N = 20 .. 32 with R = 2; (256, 16, 64) N = 20 .. 25 with R = 4; (128, 16, 64) N = 20 with R = 8
# (the ranges at table_len = 512, which a beta = 0 row has)
SIZES = (2, 3, 4, 8, 12, 13, 16, 19, 20, 24, 32)
HIST = ("energy_hist", "rung_hist")


def _ladder(R, lo=0.5, hi=2.0):
    return [float(x) for x in np.linspace(lo, hi, R)]


def _placements(N, n, seed, Q=None):
    Qn = N * N if Q is None else Q
    s = q3.random_placements(N, n, seed, Q=Q, over=seed % 2 == 1).reshape(n, Qn, 3)
    if N ** 3 - Qn >= Qn:  # chain 0: the queens in the first cells, a placement no random draw gives
        flat = np.arange(Qn)
        s[0] = np.stack([flat // (N * N), (flat // N) % N, flat % N], axis=1)
    return s.reshape(n, 3 * Qn)


def _seeds(n, k):
    s = (np.arange(n, dtype=np.uint64) * 2654435761 + k) % 2**32
    s[-1] = 2**32 - 1
    return s.astype(np.uint32)


def _rungs(n, R, seed):
    rs = np.random.RandomState(seed)
    return np.concatenate([rs.permutation(R) for _ in range(n // R)]).astype(np.uint8)


def _same(got, want, what, hist):
    t3.assert_equal(got, want, what, hist=hist)
    assert set(got) == set(want), what
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)


def _replicas(N, Q=None):
    return [R for R in abi.TEMPER_REPLICAS if t3.fits(N, R, Q)]


def test_every_instantiation_is_reached():
    lanes = lambda N, R: min(64 if N <= 12 else 256 if N <= 19 else 1024, 1024 // R)  # noqa: E731
    shapes = {(lanes(N, R), 8 if N <= 19 else 16, 32 if N <= 12 else 64): [] for N in SIZES for R in _replicas(N)}
    for N in SIZES:
        for R in _replicas(N):
            shapes[(lanes(N, R), 8 if N <= 19 else 16, 32 if N <= 12 else 64)].append(N)
    assert set(shapes) == {(64, 8, 32), (256, 8, 64), (128, 8, 64), (64, 8, 64), (512, 16, 64), (256, 16, 64), (128, 16, 64)}
    assert shapes[(64, 8, 64)] == [13, 16] and shapes[(128, 16, 64)] == [20] and shapes[(512, 16, 64)] == [20, 24, 32]
    assert [_replicas(N) for N in (12, 19, 20, 24, 32)] == [[2, 4, 8, 16], [2, 4, 8], [2, 4, 8], [2, 4], [2]]


@pytest.mark.parametrize("N", SIZES)
def test_kernel_equals_the_host_code(N):
    """Every R the LDS allows at N; 1, 2 or 3 ladders; K = 1, 2, 3; 3 to 5 sweeps (2 from N = 24 on); histories on and off; rung_in
    given and default; first_sweep off a multiple of K; a beta = 0 row (D = 512, W beyond 32 bits from N = 7 on)."""
    Q = N * N
    for idx, R in enumerate(_replicas(N)):
        ladders = (1 + (idx + N) % 3) if N < 20 else 1 + idx % 2 if N < 24 else 1
        K, T, trace = 1 + (idx + N) % 3, (3 + (idx + N) % 3) if N < 24 else 2, (idx + N) % 2 == 0
        first = (1, 4, (1 << 34) // Q + 5, 7)[(idx + N) % 4]
        first += first % K == 0 and K > 1
        betas = np.linspace(0.0, 1.5, T) if idx % 2 == 0 else np.linspace(0.3, 1.6, T)
        n = R * ladders
        s, seeds = _placements(N, n, 10 * N + idx), _seeds(n, N + idx)
        rungs = _rungs(n, R, idx) if (idx + N) % 3 else None
        what = f"N={N} R={R}, {ladders} ladders, K={K}, {T} sweeps from {first}, rung_in={'given' if rungs is not None else 'default'}"
        assert K == 1 or first % K, what
        kw = dict(exchange_every=K, first_sweep=first, rungs=rungs, trace=trace)
        want = tempering.temper_queens_host(N, s, seeds, betas, _ladder(R), **kw)
        got = tempering.temper_queens(N, s, seeds, betas, _ladder(R), **kw)
        _same(got, want, what, trace)
        assert not got["flags"].any() and got["n_changed"].all()


@pytest.mark.parametrize("N", (2, 4, 12))
def test_other_queen_counts_a_table_of_one_entry_and_no_sweep(N):
    """Q = 2 and Q = N^3 - 1 with every R (N = 12, R = 16, Q = 1727 takes 124 096 bytes of LDS); a table of one entry (uniform updates)
    through `tables`; no sweep at all."""
    import torch

    for idx, Q in enumerate((2, N ** 3 - 1)):
        for R in _replicas(N, Q):
            if N == 12 and Q > 2 and R in (4, 8):
                continue  # (2 and 16 are the ends)
            n, K, T = 2 * R if Q == 2 else R, 1 + (R + idx) % 2, 3 if Q == 2 else 2
            s, seeds = _placements(N, n, N + R + idx, Q=Q), _seeds(n, R)
            betas = np.linspace(0.2, 1.4, T)
            kw = dict(Q=Q, exchange_every=K, first_sweep=K + 1, rungs=_rungs(n, R, N), trace=True)
            _same(tempering.temper_queens(N, s, seeds, betas, _ladder(R), **kw), tempering.temper_queens_host(N, s, seeds, betas, _ladder(R), **kw),
                  f"N={N} Q={Q} R={R}", True)
    dev = torch.device("cuda", torch.cuda.current_device())
    R, n, T, Q = 2, 6, 3, N * N
    s, seeds = _placements(N, n, 7 * N), _seeds(n, 1)
    one = np.full((T, R, 1), 1 << 24, dtype=np.uint32)
    X = abi.temper_tables([0.2] * T, [1.0, 2.0])[1]
    want = t3.host_call(N, Q, s, seeds, one, X, 1, 2)
    tabs = (torch.from_numpy(one.view(np.int32)).to(dev), torch.from_numpy(X.view(np.int32)).to(dev))
    res = tempering.temper_queens_device(N, torch.from_numpy(s).to(dev), seeds, tables=tabs, first_sweep=2, trace=True)
    torch.cuda.current_stream(dev).synchronize()
    _same(tempering.to_numpy(res), want, f"N={N}, a table of one entry", True)
    _same(tempering.temper_queens(N, s, seeds, [], [1.0, 2.0], first_sweep=4, trace=True),
          tempering.temper_queens_host(N, s, seeds, [], [1.0, 2.0], first_sweep=4, trace=True), f"N={N}, no sweep", True)


def test_a_short_table_lets_a_larger_ladder_in():
    """The staged rows count against the LDS: with D well below 512 a ladder of 16 fits at N = 19 (64 lanes per chain, a lane's run of
    27 dwords = 108 cells: the longest 32-bit partial sum of any shape that fits) and a ladder of 4 at N = 26."""
    for N, R, betas in ((19, 16, (0.9, 1.3)), (26, 4, (1.1,))):
        T = abi.temper_tables(betas, _ladder(R))[0]
        assert not t3.fits(N, R) and t3.fits(N, R, None, T.shape[2]) and T.shape[2] < 64
        s, seeds = _placements(N, R, N), _seeds(R, N)
        kw = dict(exchange_every=1, first_sweep=2, trace=True)
        _same(tempering.temper_queens(N, s, seeds, betas, _ladder(R), **kw), tempering.temper_queens_host(N, s, seeds, betas, _ladder(R), **kw), f"N={N} R={R}", True)


def test_a_held_ladder_among_others():
    """One slot with two queens in one cell holds its ladder, and an all-255 slot (every queen in one cell) another; the rest run."""
    for N, R, W in ((4, 4, 64), (13, 2, 256), (16, 16, 64), (20, 8, 128)):
        Q, n, T, K = N * N, 4 * R, 3, 2
        s = _placements(N, n, N).reshape(n, Q, 3)
        s[R + R // 2, Q - 1] = s[R + R // 2, 0]
        s[3 * R] = 255
        s = s.reshape(n, -1)
        seeds, rungs = _seeds(n, 4), _rungs(n, R, N)
        kw = dict(exchange_every=K, first_sweep=1, rungs=rungs, trace=True)
        want = tempering.temper_queens_host(N, s, seeds, np.linspace(0.4, 1.2, T), _ladder(R), **kw)
        got = tempering.temper_queens(N, s, seeds, np.linspace(0.4, 1.2, T), _ladder(R), **kw)
        _same(got, want, f"N={N} R={R}", True)
        flags = got["flags"].reshape(4, R)
        assert not flags[0].any() and not flags[2].any() and (flags[1] >= abi.TEMPER3D_HELD).all() and (flags[3] >= abi.TEMPER3D_HELD).all()
        assert flags[1, R // 2] == 3 and flags[3, 0] == 3 and flags[1].sum() == 2 * R + 1 and flags[3].sum() == 2 * R + 1
        assert not got["n_changed"][R: 2 * R].any() and got["n_changed"][:R].all() and got["n_changed"][2 * R: 3 * R].all()
        np.testing.assert_array_equal(got["rung_out"][R: 2 * R], rungs[R: 2 * R])


def test_kernel_equals_the_restatement():
    for N, Q, R, K in ((3, None, 4, 1), (4, None, 2, 2), (4, 20, 16, 1)):
        n = 2 * R if R < 16 else R
        s, seeds = _placements(N, n, N, Q=Q), _seeds(n, 5)
        betas = (0.4, 1.0, 1.3)
        got = tempering.temper_queens(N, s, seeds, betas, _ladder(R), Q=Q, exchange_every=K, first_sweep=1, trace=True)
        t3.assert_equal(got, t3.run_many(N, s, seeds, betas, _ladder(R), Q, K, 1), f"N={N} R={R} vs the restatement", hist=True)


def test_device_segments_equal_the_unbroken_launch():
    """In place (state_out == state_in), first_sweep, the rungs and the placements carried on the device, the tables built per segment;
    cuts at sweeps that are and that are not followed by an event."""
    import torch

    dev = torch.device("cuda", torch.cuda.current_device())
    st = torch.cuda.current_stream(dev)
    for N, R, ladders, K, cuts, first in ((12, 16, 3, 2, (0, 2, 3, 6), 1), (16, 4, 2, 3, (0, 1, 3, 5), 0), (24, 2, 1, 2, (0, 1, 2, 3), (1 << 35) // 576)):
        n, total = R * ladders, cuts[-1]
        betas, ladder = np.linspace(0.3, 1.5, total), _ladder(R)
        s, seeds, rungs = _placements(N, n, 31 * N), _seeds(n, 3), _rungs(n, R, N)
        whole = tempering.temper_queens(N, s, seeds, betas, ladder, exchange_every=K, first_sweep=first, rungs=rungs, trace=True)
        t, rung = torch.from_numpy(s).to(dev), torch.from_numpy(rungs).to(dev)
        ehist, rhist, followed = [], [], set()
        totals = {k: 0 for k in ("n_changed", "n_exchanges", "pair_accepted")}
        for a, b in zip(cuts[:-1], cuts[1:]):
            followed.add((first + b) % K == 0)
            res = tempering.temper_queens_device(N, t, seeds, betas[a:b], ladder, exchange_every=K, first_sweep=first + a, rungs=rung, out=t, trace=True)
            assert res["state"] is t
            st.synchronize()
            rung = res["rung_out"]
            got = tempering.to_numpy(res)
            ehist.append(got["energy_hist"][:, 0 if a == 0 else 1:]), rhist.append(got["rung_hist"][:, 0 if a == 0 else 1:])
            for k in totals:
                totals[k] = totals[k] + got[k]
        what = f"N={N} R={R} K={K} cuts {cuts}"
        assert followed == {True, False}, what
        np.testing.assert_array_equal(t.cpu().numpy(), whole["state"], err_msg=what)
        np.testing.assert_array_equal(got["rung_out"], whole["rung_out"], err_msg=what)
        np.testing.assert_array_equal(got["energy_out"], whole["energy_out"], err_msg=what)
        np.testing.assert_array_equal(np.concatenate(ehist, axis=1), whole["energy_hist"], err_msg=what)
        np.testing.assert_array_equal(np.concatenate(rhist, axis=1), whole["rung_hist"], err_msg=what)
        for k in totals:
            np.testing.assert_array_equal(totals[k], whole[k], err_msg=f"{what}: {k}")


def test_a_ladder_of_equal_multipliers_is_the_heatbath_kernel():
    """The new kernel against the old one: R equal rows are R plain full_3d heat-bath chains, whatever the exchanges do."""
    for N, R, ladders, K in ((8, 2, 5, 1), (12, 16, 2, 2), (19, 4, 2, 1), (20, 8, 1, 3), (32, 2, 1, 1)):
        n = R * ladders
        s, seeds = _placements(N, n, N + R), _seeds(n, R)
        betas = np.linspace(0.5, 2.0, 4 if N < 32 else 2)
        got = tempering.temper_queens(N, s, seeds, betas, [1.25] * R, exchange_every=K, first_sweep=3, trace=True)
        want = heatbath.heatbath_queens(N, s, seeds, betas * 1.25, first_sweep=3, trace=True)
        for k in heatbath.FIELDS + ("energy_hist",):
            np.testing.assert_array_equal(got[k], want[k], err_msg=f"N={N} R={R}: {k}")
        assert got["n_exchanges"].sum() > 0


def test_one_wide_launch():
    """N = 12, 1 024 ladders of 16, 3 sweeps, K = 1: energy_out and best_energy against the full_3d quench kernel's recount of state and
    best_state, the exchange's invariants over all ladders, and three sampled ladders against the host code."""
    import torch

    N, R, L, K = 12, 16, 1024, 1
    n, betas, ladder = R * L, np.linspace(0.5, 1.5, 3), _ladder(R, 0.4, 2.0)
    s, seeds = q3.random_placements(N, n, 12), abi.seeds_for(42, n)
    dev = torch.device("cuda", torch.cuda.current_device())
    res = tempering.temper_queens_device(N, torch.from_numpy(s).to(dev), seeds, betas, ladder, exchange_every=K, trace=True)
    again = quench.quench_queens_device(N, res["state"], max_passes=1, conflicts=False)
    best = quench.quench_queens_device(N, res["best_state"], max_passes=1, conflicts=False)
    torch.cuda.current_stream(dev).synchronize()
    got = tempering.to_numpy(res)
    np.testing.assert_array_equal(again["energy_in"].cpu().numpy(), got["energy_out"], err_msg="the quench kernel's recount of state_out")
    np.testing.assert_array_equal(best["energy_in"].cpu().numpy(), got["best_energy"], err_msg="the quench kernel's recount of best_state")
    np.testing.assert_array_equal(got["energy_hist"].min(axis=1), got["best_energy"])
    np.testing.assert_array_equal(got["energy_hist"].argmin(axis=1), got["best_sweep"])
    assert not got["flags"].any()
    t3.check_invariants(got, R, K, 0)
    pick = np.r_[0: R, n // 2: n // 2 + R, n - R: n]
    want = tempering.temper_queens_host(N, s[pick], seeds[pick], betas, ladder, exchange_every=K, trace=True)
    lad = pick[::R] // R
    t3.assert_equal(dict({k: v[pick] for k, v in got.items() if k != "pair_accepted"}, pair_accepted=got["pair_accepted"][lad]), want,
                    "three of 1 024 ladders", hist=True)
    rate = got["pair_accepted"].sum(axis=0) / (L * np.array([2 if t % 2 == 0 else 1 for t in range(R - 1)]))  # three events: 0, 1, 2
    print("N=12, 1 024 ladders of 16, 3 sweeps: accepted share per pair of rungs", np.round(rate, 3))
    assert got["pair_accepted"].sum() > 0 and (rate <= 1.0).all()


def test_temper_queens_device_on_a_stream_of_its_own():
    import torch

    dev = torch.device("cuda", torch.cuda.current_device())
    N, R, ladders, K, first = 13, 4, 5, 2, 3
    n, betas, ladder = R * ladders, np.linspace(0.4, 1.4, 4), _ladder(R)
    s, seeds, rungs = _placements(N, n, 5), _seeds(n, 9), _rungs(n, R, 2)
    want = tempering.temper_queens_host(N, s, seeds, betas, ladder, exchange_every=K, first_sweep=first, rungs=rungs, trace=True)
    st = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(st):
        t = torch.from_numpy(s.reshape(n, N * N, 3)).to(dev)  # [n][Q][3]
        dseeds = torch.from_numpy(seeds.view(np.int32)).to(dev)
        drungs = torch.from_numpy(rungs).to(dev)
        tabs = tempering.device_tables(betas, ladder, K, first, dev)
    st.synchronize()
    kw = dict(tables=tabs, exchange_every=K, first_sweep=first, rungs=drungs, stream=st)
    res = tempering.temper_queens_device(N, t, dseeds, trace=True, **kw)
    st.synchronize()
    assert res["state"].shape == t.shape and res["best_state"].shape == t.shape
    got = tempering.to_numpy(res)
    got["state"], got["best_state"] = got["state"].reshape(n, -1), got["best_state"].reshape(n, -1)
    _same(got, want, "tables, seeds and rungs as tensors, own stream", True)
    lean = tempering.temper_queens_device(N, t, dseeds, best_state=False, **kw)
    st.synchronize()
    assert "best_state" not in lean and "energy_hist" not in lean
    t3.assert_equal(tempering.to_numpy(lean), want, "without best_state", fields=[k for k in t3.FIELDS if k != "best_state"])
    for bad, msg in ((dict(tables=(tabs[0], tabs[1][:, :1].contiguous())), "pairs of rungs"), (dict(tables=(tabs[0].long(), tabs[1])), "int32"),
                     (dict(tables=tabs, rungs=drungs[:4]), "rungs"), (dict(), "betas and ladder"), (dict(tables=tabs, Q=100), "final_state layout of full_3d"),
                     (dict(tables=tabs, out=t[:4]), "out must be")):
        with pytest.raises(ValueError, match=msg):
            tempering.temper_queens_device(N, t, dseeds, **dict(dict(exchange_every=K, first_sweep=first), **bad))
    with pytest.raises(ValueError, match="takes 172736 bytes of LDS"):
        tempering.temper_queens(19, _placements(19, 16, 1), _seeds(16, 1), [0.0], _ladder(16))  # (beta = 0: a row of 512 entries)
    with pytest.raises(ValueError, match="no permutation|permutation of 0"):
        tempering.temper_queens(4, _placements(4, 4, 1), _seeds(4, 1), [1.0], _ladder(2), rungs=[0, 0, 1, 0])


def test_anneal_tempered_equals_the_run_composed_on_the_host():
    lin = {"type": "linear_annealing", "beta_start": 0.5, "beta_end": 2.0}
    N, R, K, T = 8, 8, 2, 5
    ladder = _ladder(R, 0.5, 1.5)
    seeds = abi.seeds_for(42, 2 * R)
    for init, Q in (("random", None), (_placements(N, 2 * R, 3, Q=40), 40)):
        res = tempering.anneal_tempered(N, T, init, lin, seeds, ladder, exchange_every=K, quench=True, trace=True, mcmc_type="full_3d", Q=Q)
        if isinstance(init, str):
            first, _ = mcq_amd.experiments.start_chains(N, 0, init, lin, seeds, mcmc_type="full_3d", trace=False, states=True, Q=N * N)
            start = np.ascontiguousarray(first["final_state"], dtype=np.uint8).reshape(len(seeds), -1)
        else:
            start = init
        want = tempering.temper_queens_host(N, start, seeds, abi.beta_values(lin, T), ladder, Q=Q, exchange_every=K, trace=True)
        for a, b in (("initial_energy", "energy_in"), ("final_energy", "energy_out"), ("final_state", "state"), ("final_rung", "rung_out")) + \
                tuple((k, k) for k in ("best_energy", "best_sweep", "best_state", "n_changed", "n_exchanges", "pair_accepted", "flags") + HIST):
            np.testing.assert_array_equal(res[a], want[b], err_msg=a)
        q = quench.quench_queens_host(N, want["best_state"], Q=Q, conflicts=False)
        np.testing.assert_array_equal(res["quenched_state"], q["state"])
        np.testing.assert_array_equal(res["quenched_energy"], q["energy_out"])
        np.testing.assert_array_equal(res["quench_moves"], q["n_moves"])
        offers = np.array([len([e for e in range(T // K) if e % 2 == t % 2]) for t in range(R - 1)]) * 2
        with np.errstate(divide="ignore", invalid="ignore"):
            np.testing.assert_allclose(res["pair_rate"], np.where(offers > 0, want["pair_accepted"].sum(axis=0) / offers, 0.0))
    with pytest.raises(ValueError, match="must divide"):
        tempering.anneal_tempered(N, T, "random", lin, seeds[:5], ladder, mcmc_type="full_3d")
