"""GPU: the tempering kernel (mcq_temper_device) against the library's host code (mcq_temper_host) bit for bit on every output and
every instantiation, device segments against the unbroken launch, a ladder of equal multipliers against the plain heat-bath kernel, one
wide launch against the quench kernel's recount and the exchange's invariants, temper_device on torch tensors on a stream of its own,
and anneal_tempered against the same run composed on the host."""
import numpy as np
import pytest

import mcq_amd
from tests import quench_util as qu
from tests import temper_util as tu

abi = mcq_amd.abi
heatbath = mcq_amd.heatbath
quench = mcq_amd.quench
tempering = mcq_amd.tempering
pytestmark = pytest.mark.gpu

# every instantiation (line paddings 8, 12, 16, 24, 32, 64; 16, 32, 64 lanes per chain)
SIZES = (2, 3, 8, 12, 13, 16, 17, 24, 32, 33, 64)
HIST = ("energy_hist", "rung_hist")


def _ladder(R, lo=0.5, hi=2.0):
    return [float(x) for x in np.linspace(lo, hi, R)]


def _boards(N, n, seed):
    s = qu.random_boards(N, n, seed, over=seed % 2 == 1)
    s[0] = seed % N  # all heights equal
    if n > 2:
        s[1] = 255  # clamped
    return s


def _seeds(n, k):
    s = (np.arange(n, dtype=np.uint64) * 2654435761 + k) % 2**32
    s[-1] = 2**32 - 1
    return s.astype(np.uint32)


def _rungs(n, R, seed):
    rs = np.random.RandomState(seed)
    return np.concatenate([rs.permutation(R) for _ in range(n // R)]).astype(np.uint8)


def _same(got, want, what, hist):
    tu.assert_equal(got, want, what, hist=hist)
    assert set(got) == set(want), what
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)


@pytest.mark.parametrize("N", SIZES)
def test_kernel_equals_the_host_code(N):
    """Every R the LDS allows at N; 1, 2 and 3 ladders (two ladders share a workgroup for R = 2 at N <= 16: the odd counts leave half
    of one empty); K = 1, 2, 3; 5 to 7 sweeps; histories on and off; first_sweep off a multiple of K; a beta = 0 row (D = 512)."""
    idx = 0
    for R in (2, 4, 8, 16) if N <= 32 else (2, 4):
        for ladders in (1, 2, 3):
            K, T, trace = 1 + idx % 3, 5 + idx % 3, idx % 2 == 0
            first = (1, 4, (1 << 34) // (N * N) + 5, 7)[idx % 4]
            first += first % K == 0 and K > 1
            betas = np.linspace(0.0, 1.5, T) if idx % 4 == 1 else np.linspace(0.3, 1.6, T)
            n = R * ladders
            s, seeds = _boards(N, n, 10 * N + idx), _seeds(n, N + idx)
            rungs = _rungs(n, R, idx) if idx % 3 else None
            what = f"N={N} R={R}, {ladders} ladders, K={K}, {T} sweeps from {first}, rung_in={'given' if idx % 3 else 'default'}"
            assert K == 1 or first % K, what
            want = tempering.temper_states_host(N, s, seeds, betas, _ladder(R), exchange_every=K, first_sweep=first, rungs=rungs, trace=trace)
            got = tempering.temper_states(N, s, seeds, betas, _ladder(R), exchange_every=K, first_sweep=first, rungs=rungs, trace=trace)
            _same(got, want, what, trace)
            idx += 1
    # a table of one entry (uniform updates) with the caller's own tables, and no sweep at all
    import torch

    dev = torch.device("cuda", torch.cuda.current_device())
    R, n, T = 2, 6, 3
    s, seeds = _boards(N, n, 7 * N), _seeds(n, 1)
    one = np.full((T, R, 1), 1 << 24, dtype=np.uint32)
    X = abi.temper_tables([0.2] * T, [1.0, 2.0])[1]
    want = tu.host_call(N, s, seeds, one, X, 1, 2)
    tabs = (torch.from_numpy(one.view(np.int32)).to(dev), torch.from_numpy(X.view(np.int32)).to(dev))
    res = tempering.temper_device(N, torch.from_numpy(s).to(dev), seeds, tables=tabs, first_sweep=2, trace=True)
    torch.cuda.current_stream(dev).synchronize()
    _same(tempering.to_numpy(res), want, f"N={N}, a table of one entry", True)
    _same(tempering.temper_states(N, s, seeds, [], [1.0, 2.0], first_sweep=4, trace=True),
          tempering.temper_states_host(N, s, seeds, [], [1.0, 2.0], first_sweep=4, trace=True), f"N={N}, no sweep", True)


def test_kernel_equals_the_restatement():
    for N, R, K in ((3, 4, 1), (8, 2, 2), (12, 16, 1), (17, 2, 1)):
        n = 2 * R if N < 12 else R
        s, seeds = _boards(N, n, N), _seeds(n, 5)
        betas = (0.4, 1.0, 1.3)
        got = tempering.temper_states(N, s, seeds, betas, _ladder(R), exchange_every=K, first_sweep=1, trace=True)
        tu.assert_equal(got, tu.run_many(N, s, seeds, betas, _ladder(R), K, 1), f"N={N} R={R} vs the restatement", hist=True)


def test_device_segments_equal_the_unbroken_launch():
    """In place (state_out == state_in), first_sweep, the rungs and the placements carried on the device, the tables built per segment;
    cuts at sweeps that are and that are not followed by an event."""
    import torch

    dev = torch.device("cuda", torch.cuda.current_device())
    st = torch.cuda.current_stream(dev)
    for N, R, ladders, K, cuts, first in ((12, 16, 3, 2, (0, 2, 3, 7), 1), (13, 2, 5, 3, (0, 1, 3, 6), 0), (24, 8, 2, 2, (0, 1, 4), (1 << 35) // 576), (40, 4, 1, 1, (0, 2, 3), 5)):
        n, total = R * ladders, cuts[-1]
        betas, ladder = np.linspace(0.3, 1.5, total), _ladder(R)
        s, seeds, rungs = _boards(N, n, 31 * N), _seeds(n, 3), _rungs(n, R, N)
        whole = tempering.temper_states(N, s, seeds, betas, ladder, exchange_every=K, first_sweep=first, rungs=rungs, trace=True)
        t, rung = torch.from_numpy(s).to(dev), torch.from_numpy(rungs).to(dev)
        ehist, rhist = [], []
        totals = {k: 0 for k in ("n_changed", "n_exchanges", "pair_accepted")}
        for a, b in zip(cuts[:-1], cuts[1:]):
            res = tempering.temper_device(N, t, seeds, betas[a:b], ladder, exchange_every=K, first_sweep=first + a, rungs=rung, out=t, trace=True)
            assert res["state"] is t
            st.synchronize()
            rung = res["rung_out"]
            got = tempering.to_numpy(res)
            ehist.append(got["energy_hist"][:, 0 if a == 0 else 1:]), rhist.append(got["rung_hist"][:, 0 if a == 0 else 1:])
            for k in totals:
                totals[k] = totals[k] + got[k]
        what = f"N={N} R={R} K={K} cuts {cuts}"
        np.testing.assert_array_equal(t.cpu().numpy(), whole["state"], err_msg=what)
        np.testing.assert_array_equal(got["rung_out"], whole["rung_out"], err_msg=what)
        np.testing.assert_array_equal(got["energy_out"], whole["energy_out"], err_msg=what)
        np.testing.assert_array_equal(np.concatenate(ehist, axis=1), whole["energy_hist"], err_msg=what)
        np.testing.assert_array_equal(np.concatenate(rhist, axis=1), whole["rung_hist"], err_msg=what)
        for k in totals:
            np.testing.assert_array_equal(totals[k], whole[k], err_msg=f"{what}: {k}")


def test_a_ladder_of_equal_multipliers_is_the_heatbath_kernel():
    """The new kernel against the old one: R equal rows are R plain heat-bath chains, whatever the exchanges do."""
    for N, R, ladders, K in ((8, 2, 5, 1), (12, 16, 3, 2), (16, 4, 2, 1), (24, 8, 2, 3), (32, 16, 1, 1), (64, 4, 1, 2)):
        n = R * ladders
        s, seeds = _boards(N, n, N + R), _seeds(n, R)
        betas = np.linspace(0.5, 2.0, 4)
        got = tempering.temper_states(N, s, seeds, betas, [1.25] * R, exchange_every=K, first_sweep=3, trace=True)
        want = heatbath.heatbath_states(N, s, seeds, betas * 1.25, first_sweep=3, trace=True)
        for k in heatbath.FIELDS + ("energy_hist",):
            np.testing.assert_array_equal(got[k], want[k], err_msg=f"N={N} R={R}: {k}")
        assert got["n_exchanges"].sum() > 0


def test_one_wide_launch():
    """N = 12, 4 096 ladders of 16, 4 sweeps, K = 1: energy_out and best_energy against the quench kernel's recount of state and
    best_state, the exchange's invariants over all ladders, and a sample of ladders against the host code."""
    import torch

    N, R, L, K = 12, 16, 4096, 1
    n, betas, ladder = R * L, np.linspace(0.5, 1.5, 4), _ladder(R, 0.4, 2.0)
    s, seeds = qu.random_boards(N, n, 12), abi.seeds_for(42, n)
    dev = torch.device("cuda", torch.cuda.current_device())
    res = tempering.temper_device(N, torch.from_numpy(s).to(dev), seeds, betas, ladder, exchange_every=K, trace=True)
    again = quench.quench_device(N, res["state"], max_passes=1, conflicts=False)
    best = quench.quench_device(N, res["best_state"], max_passes=1, conflicts=False)
    torch.cuda.current_stream(dev).synchronize()
    got = tempering.to_numpy(res)
    np.testing.assert_array_equal(again["energy_in"].cpu().numpy(), got["energy_out"], err_msg="the quench kernel's recount of state_out")
    np.testing.assert_array_equal(best["energy_in"].cpu().numpy(), got["best_energy"], err_msg="the quench kernel's recount of best_state")
    np.testing.assert_array_equal(got["energy_hist"].min(axis=1), got["best_energy"])
    np.testing.assert_array_equal(got["energy_hist"].argmin(axis=1), got["best_sweep"])
    tu.check_invariants(got, R, K, 0)
    pick = np.r_[0: 2 * R, n // 2: n // 2 + 2 * R, n - 2 * R: n]
    want = tempering.temper_states_host(N, s[pick], seeds[pick], betas, ladder, exchange_every=K, trace=True)
    lad = pick[::R] // R
    tu.assert_equal(dict({k: v[pick] for k, v in got.items() if k != "pair_accepted"}, pair_accepted=got["pair_accepted"][lad]), want,
                    "a sample of 4 096 ladders", hist=True)
    rate = got["pair_accepted"].sum(axis=0) / (L * 2)  # four events: two offers to every pair
    print("N=12, 4 096 ladders of 16, 4 sweeps: accepted share per pair of rungs", np.round(rate, 3))
    assert got["pair_accepted"].sum() > 0 and (rate <= 1.0).all()


def test_temper_device_on_a_stream_of_its_own():
    import torch

    dev = torch.device("cuda", torch.cuda.current_device())
    N, R, ladders, K, first = 13, 4, 9, 2, 3
    n, betas, ladder = R * ladders, np.linspace(0.4, 1.4, 6), _ladder(R)
    s, seeds, rungs = _boards(N, n, 5), _seeds(n, 9), _rungs(n, R, 2)
    want = tempering.temper_states_host(N, s, seeds, betas, ladder, exchange_every=K, first_sweep=first, rungs=rungs, trace=True)
    st = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(st):
        t = torch.from_numpy(s).to(dev)
        dseeds = torch.from_numpy(seeds.view(np.int32)).to(dev)
        drungs = torch.from_numpy(rungs).to(dev)
        tabs = tempering.device_tables(betas, ladder, K, first, dev)
    st.synchronize()
    res = tempering.temper_device(N, t, dseeds, tables=tabs, exchange_every=K, first_sweep=first, rungs=drungs, trace=True, stream=st)
    st.synchronize()
    _same(tempering.to_numpy(res), want, "tables, seeds and rungs as tensors, own stream", True)
    lean = tempering.temper_device(N, t, dseeds, tables=tabs, exchange_every=K, first_sweep=first, rungs=drungs, best_state=False, stream=st)
    st.synchronize()
    assert "best_state" not in lean and "energy_hist" not in lean
    tu.assert_equal(tempering.to_numpy(lean), want, "without best_state", fields=[k for k in tu.FIELDS if k != "best_state"])
    for bad, msg in ((dict(tables=(tabs[0], tabs[1][:, :1].contiguous())), "pairs of rungs"), (dict(tables=(tabs[0].long(), tabs[1])), "int32"),
                     (dict(tables=tabs, rungs=drungs[:4]), "rungs"), (dict(), "betas and ladder")):
        with pytest.raises(ValueError, match=msg):
            tempering.temper_device(N, t, dseeds, **dict(dict(exchange_every=K, first_sweep=first), **bad))
    with pytest.raises(ValueError, match="bytes of LDS"):
        tempering.temper_states(64, _boards(64, 8, 1), _seeds(8, 1), [1.0], _ladder(8))


def test_anneal_tempered_equals_the_run_composed_on_the_host():
    lin = {"type": "linear_annealing", "beta_start": 0.5, "beta_end": 2.0}
    N, R, K, T = 12, 8, 2, 9
    ladder = _ladder(R, 0.5, 1.5)
    seeds = abi.seeds_for(42, 4 * R)
    for init in ("random", _boards(N, 4 * R, 3)):
        res = tempering.anneal_tempered(N, T, init, lin, seeds, ladder, exchange_every=K, quench=True, trace=True)
        if isinstance(init, str):
            first, _ = mcq_amd.experiments.start_chains(N, 0, init, lin, seeds, mcmc_type="board", trace=False, states=True)
            start = np.ascontiguousarray(first["final_state"], dtype=np.uint8).reshape(len(seeds), -1)
        else:
            start = init
        want = tempering.temper_states_host(N, start, seeds, abi.beta_values(lin, T), ladder, exchange_every=K, trace=True)
        for a, b in (("initial_energy", "energy_in"), ("final_energy", "energy_out"), ("final_state", "state"), ("final_rung", "rung_out")) + \
                tuple((k, k) for k in ("best_energy", "best_sweep", "best_state", "n_changed", "n_exchanges", "pair_accepted") + HIST):
            np.testing.assert_array_equal(res[a], want[b], err_msg=a)
        q = quench.quench_states_host(N, want["best_state"], conflicts=False)
        np.testing.assert_array_equal(res["quenched_state"], q["state"])
        np.testing.assert_array_equal(res["quenched_energy"], q["energy_out"])
        np.testing.assert_array_equal(res["quench_moves"], q["n_moves"])
        offers = np.array([len([e for e in range(T // K) if e % 2 == t % 2]) for t in range(R - 1)]) * 4
        np.testing.assert_allclose(res["pair_rate"], want["pair_accepted"].sum(axis=0) / offers)
    with pytest.raises(ValueError, match="must divide"):
        tempering.anneal_tempered(N, T, "random", lin, seeds[:5], ladder)
    with pytest.raises(ValueError, match="non-decreasing"):
        tempering.anneal_tempered(N, T, "random", lin, seeds, ladder[::-1])
