"""CPU-only: the tempering rule in host code (mcq_temper_host) against its NumPy restatement (tests/temper_util.py) on every output,
against the plain heat-bath host code where the two must agree, the invariants of the exchange, segments, the stationary distribution of
every rung on a board small enough to enumerate, every refusal, and the layout of the mcq_temper block."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

import mcq_amd
from tests import heatbath_util as hu
from tests import quench_util as qu
from tests import temper_util as tu

abi = mcq_amd.abi
heatbath = mcq_amd.heatbath
tempering = mcq_amd.tempering
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = 1 << 34


def ladder_of(R, lo=0.5, hi=1.5):
    return [float(x) for x in np.linspace(lo, hi, R)]


def permuted_rungs(n, R, seed):
    rs = np.random.RandomState(seed)
    return np.concatenate([rs.permutation(R) for _ in range(n // R)]).astype(np.uint8)


def test_table_builder():
    for betas, ladder, K, first in (([1.0, 2.0, 0.5], [0.5, 1.0], 1, 0), ([0.3] * 7, [0.25, 0.5, 1.0, 2.0], 3, 4), ([0.0, 1.0], [1.0, 1.0], 1, 0),
                                    ([2.0] * 5, ladder_of(8), 2, 1), ([], [1.0, 2.0], 1, 0), ([1.0, 1.5], ladder_of(16), 5, 0), ([0.0, 0.0], [1.0, 3.0], 1, 9)):
        T, X = abi.temper_tables(betas, ladder, K, first)
        wT, wX = tu.tables(betas, ladder, K, first)
        assert T.dtype == X.dtype == np.uint32 and T.flags.c_contiguous and X.flags.c_contiguous
        np.testing.assert_array_equal(T, wT, err_msg=str((betas, ladder)))
        np.testing.assert_array_equal(X, wX, err_msg=str((betas, ladder, K, first)))
        assert X.shape[0] == abi.temper_events(first, len(betas), K) == tu.events(first, len(betas), K) and X.shape[1] == len(ladder) - 1
        for s, b in enumerate(betas):  # a rung's rows are heatbath_table's at beta times its multiplier
            for t, l in enumerate(ladder):
                row = abi.heatbath_table([b * l])[0]
                np.testing.assert_array_equal(T[s, t, : len(row)], row[: T.shape[2]])
    T, X = abi.temper_tables([1.0], [1.0, 2.0])
    assert X.shape == (1, 1, 24) and X[0, 0, 0] == 2**32 - 1 and X[0, 0, 1] == int(np.floor(2.0**32 * np.exp(-1.0))) and X[0, 0, 22] == 1 and X[0, 0, 23] == 0
    assert abi.temper_tables([1.0], [1.0, 1.0])[1].shape == (1, 1, 1)  # equal multipliers: a constant row reads the same at any length


def test_pythons_refusals():
    for bad, msg in (([1.0, 0.5], "non-decreasing"), ([0.0, 1.0], "positive"), ([-1.0, 1.0], "positive"), ([1.0, float("inf")], "finite"),
                     ([1.0, float("nan")], "finite"), ([1.0, 2.0, 3.0], "2, 4, 8 or 16"), ([1.0], "2, 4, 8 or 16"), ([1.0] * 32, "2, 4, 8 or 16")):
        with pytest.raises(ValueError, match=msg):
            abi.temper_tables([1.0], bad)
    with pytest.raises(ValueError, match=r"l\[1\] - l\[0\] = 0.001.*too small"):  # exp(-0.001 d) is far from 0 at d = 4095
        abi.temper_tables([1.0, 1.0], [1.0, 1.001])
    with pytest.raises(ValueError, match="too small"):
        abi.temper_tables([3.0, 0.001], [1.0, 2.0])
    abi.temper_tables([3.0, 0.001], [1.0, 2.0], exchange_every=2, first_sweep=1)  # the event follows the sweep at beta = 3
    abi.temper_tables([1.0], [1.0, 1.006])  # 4095 * 0.006 = 24.6 > 32 ln 2
    with pytest.raises(ValueError, match="beta >= 0"):
        abi.temper_tables([-1.0], [1.0, 2.0])
    with pytest.raises(ValueError, match="exchange_every"):
        abi.temper_tables([1.0], [1.0, 2.0], exchange_every=0)
    with pytest.raises(ValueError, match="first_sweep"):
        abi.temper_tables([1.0], [1.0, 2.0], first_sweep=-1)
    boards = qu.random_boards(6, 4, 1)
    with pytest.raises(ValueError, match="non-decreasing"):
        tempering.temper_states_host(6, boards, [1, 2, 3, 4], [1.0], [2.0, 1.0])
    with pytest.raises(ValueError, match="one entry per chain"):
        tempering.temper_states_host(6, boards, [1, 2, 3, 4], [1.0], [1.0, 2.0], rungs=[0, 1])
    with pytest.raises(ValueError, match="must divide"):
        tempering.temper_states_host(6, boards[:3], [1, 2, 3], [1.0], [1.0, 2.0])
    with pytest.raises(ValueError, match="no permutation"):
        tempering.temper_states_host(6, boards, [1, 2, 3, 4], [1.0], [1.0, 2.0], rungs=[0, 1, 1, 1])
    with pytest.raises(ValueError, match="n_chains"):
        tempering.temper_states_host(6, np.zeros((0, 36), dtype=np.uint8), [], [1.0], [1.0, 2.0])


# (N, R, ladders, K, first_sweep, sweeps, rung_in given)
CASES = [(2, 16, 2, 1, 0, 6, False), (3, 8, 2, 2, 3, 5, True), (8, 4, 1, 3, 4, 5, True), (12, 2, 2, 1, BIG // 144 + 5, 3, False),
         (13, 4, 1, 2, 1, 3, True), (17, 2, 1, 3, 2, 3, False), (3, 2, 3, 1, BIG // 9 + 1, 4, True), (2, 4, 2, 3, BIG // 4 + 2, 7, False),
         (8, 16, 1, 2, 1, 3, True), (12, 8, 1, 1, 0, 2, False), (3, 4, 2, 2, 0, 1, False), (2, 2, 1, 1, 7, 0, True)]


def test_host_code_equals_the_restatement():
    taken = refused = 0
    seen = set()
    for idx, (N, R, ladders, K, first, T, given) in enumerate(CASES):
        n = R * ladders
        s = qu.random_boards(N, n, 7000 + idx, over=idx % 2 == 0)
        if idx % 3 == 0:
            s[-1] = 255  # every byte clamped to N - 1
        seeds = [(1237 * idx + 77 * r) % 2**32 for r in range(n)]
        seeds[0] = 2**32 - 1 - idx
        betas = list(np.linspace(0.2, 1.2, T))
        ladder = ladder_of(R, 0.5, 2.0)
        rungs = permuted_rungs(n, R, idx) if given else None
        what = f"N={N} R={R} K={K} first_sweep={first} sweeps={T} rung_in={'given' if given else 'default'}"
        want = tu.run_many(N, s, seeds, betas, ladder, K, first, rungs)
        got = tempering.temper_states_host(N, s, seeds, betas, ladder, exchange_every=K, first_sweep=first, rungs=rungs, trace=True)
        tu.assert_equal(got, want, what, hist=True)
        assert got["rung_out"].dtype == got["rung_hist"].dtype == np.uint8 and got["n_exchanges"].dtype == got["pair_accepted"].dtype == np.int64
        assert got["pair_accepted"].shape == (ladders, R - 1) and int(got["state"].max()) < N
        plain = tempering.temper_states_host(N, s, seeds, betas, ladder, exchange_every=K, first_sweep=first, rungs=rungs)  # histories off
        assert "energy_hist" not in plain and "rung_hist" not in plain
        tu.assert_equal(plain, want, what + " without the histories")
        for draws in want["draws"]:
            for e, t, delta, x, swap in draws:
                seen.add((N, R, K))
                taken += x is not None and swap
                refused += x is not None and not swap
    assert taken >= 5 and refused >= 5, (taken, refused)  # the table decided both ways
    assert {c[0] for c in seen} == {2, 3, 8, 12, 13, 17} and {c[1] for c in seen} == {2, 4, 8, 16} and {c[2] for c in seen} == {1, 2, 3}


def test_equal_multipliers_are_plain_heatbath_chains():
    """R equal rows: every heatbath.FIELDS output is heatbath_states_host's with the same seeds and betas, whatever the exchanges do."""
    for N, R, K, first in ((6, 4, 1, 0), (12, 16, 2, 3), (17, 2, 1, 5), (33, 8, 3, 1)):
        n = 2 * R
        s = qu.random_boards(N, n, N, over=True)
        seeds = abi.seeds_for(500 + N, n)
        betas = np.linspace(0.5, 2.0, 4)
        got = tempering.temper_states_host(N, s, seeds, betas, [0.75] * R, exchange_every=K, first_sweep=first, trace=True)
        want = heatbath.heatbath_states_host(N, s, seeds, betas * 0.75, first_sweep=first, trace=True)
        for k in heatbath.FIELDS + ("energy_hist",):
            np.testing.assert_array_equal(got[k], want[k], err_msg=f"N={N} R={R}: {k}")
        assert got["n_exchanges"].sum() > 0  # and the rungs did move


def test_without_an_event_each_slot_follows_its_own_rung():
    for N, R in ((5, 4), (12, 8), (16, 2)):
        n, T = 2 * R, 3
        s = qu.random_boards(N, n, 11 * N)
        seeds = abi.seeds_for(9, n)
        betas, ladder = np.array([0.4, 1.0, 1.6]), ladder_of(R)
        rungs = permuted_rungs(n, R, N)
        got = tempering.temper_states_host(N, s, seeds, betas, ladder, exchange_every=T + 1, rungs=rungs, trace=True)
        assert not got["n_exchanges"].any() and not got["pair_accepted"].any() and (got["rung_hist"] == rungs[:, None]).all()
        np.testing.assert_array_equal(got["rung_out"], rungs)
        for r in range(n):
            want = heatbath.heatbath_states_host(N, s[r: r + 1], seeds[r: r + 1], betas * ladder[rungs[r]], trace=True)
            for k in heatbath.FIELDS + ("energy_hist",):
                np.testing.assert_array_equal(got[k][r: r + 1], want[k], err_msg=f"N={N} slot {r}: {k}")


def test_invariants_on_random_cases():
    rs = np.random.RandomState(123)
    for idx, (N, R) in enumerate(((2, 16), (3, 4), (5, 8), (8, 2), (12, 16), (13, 4), (17, 8), (24, 2))):
        K, first, T = 1 + idx % 3, int(rs.randint(0, 9)), 8
        n = R * (6 if N <= 8 else 2)
        s = qu.random_boards(N, n, 900 + idx, over=idx % 2 == 1)
        seeds = rs.randint(0, 2**32, size=n, dtype=np.uint64)
        betas = rs.uniform(0.1, 1.5, size=T)
        rungs = permuted_rungs(n, R, idx) if idx % 2 else None
        got = tempering.temper_states_host(N, s, seeds, betas, ladder_of(R, 0.4, 2.0), exchange_every=K, first_sweep=first, rungs=rungs, trace=True)
        tu.check_invariants(got, R, K, first)
        recount = mcq_amd.quench.quench_states_host(N, got["state"], max_passes=1, conflicts=False)["energy_in"]
        np.testing.assert_array_equal(got["energy_out"], recount)
        np.testing.assert_array_equal(got["best_energy"], got["energy_hist"].min(axis=1))
        np.testing.assert_array_equal(got["best_sweep"], got["energy_hist"].argmin(axis=1))
        # a swap table of zeros: x < 0 never holds, so a pair swaps exactly when Delta >= 0
        Tt, X = abi.temper_tables(betas, ladder_of(R, 0.4, 2.0), K, first)
        zero = tu.host_call(N, s, seeds, Tt, np.zeros_like(X) if X.size else np.zeros((1, R - 1, 1), dtype=np.uint32), K, first, rungs)
        tu.check_invariants(zero, R, K, first, swap_zero=True)


def test_the_pairs_word_is_the_one_the_rule_names():
    """Key word 3, the seed of the ladder's slot 0, word e R + t: recomputed here with the oracle's Philox, and the decision with it."""
    from oracle import oracle

    N, R, K, first, T = 4, 4, 2, 5, 12
    n = 3 * R
    s = qu.random_boards(N, n, 31)
    seeds = np.array([(4000000000 + 17 * r) % 2**32 for r in range(n)], dtype=np.uint32)
    betas, ladder = np.full(T, 0.6), [0.5, 1.0, 1.5, 2.0]
    Tt, X = abi.temper_tables(betas, ladder, K, first)
    got = tempering.temper_states_host(N, s, seeds, betas, ladder, exchange_every=K, first_sweep=first, trace=True)
    rh, eh = got["rung_hist"].astype(int).reshape(3, R, -1), got["energy_hist"].astype(int).reshape(3, R, -1)
    looked = 0
    for g in range(3):
        for sw in range(T):
            if (first + sw + 1) % K:
                continue
            e = (first + sw + 1) // K - 1
            j = e - first // K
            slot_of = np.argsort(rh[g, :, sw])
            for t in range(e % 2, R - 1, 2):
                a, b = slot_of[t], slot_of[t + 1]
                delta = eh[g, b, sw + 1] - eh[g, a, sw + 1]
                swapped = rh[g, a, sw + 1] == t + 1
                if delta >= 0:
                    assert swapped
                    continue
                w = e * R + t
                x = int(oracle.philox_block([(w >> 2) & 0xFFFFFFFF, w >> 34, 0, 0], [int(seeds[g * R]), 3])[w & 3])
                assert x == tu.exchange_word(int(seeds[g * R]), w)
                assert swapped == (x < int(X[j, t, min(-delta, X.shape[2] - 1)])), (g, sw, t)
                looked += 1
    assert looked >= 10


def test_segments_equal_the_unbroken_call():
    """Cut at a sweep that is followed by an event and at one that is not: first_sweep, the rungs and the placements carried over, the
    swap table's rows split where the cut falls."""
    for N, R, K, first, total, cuts in ((6, 4, 2, 1, 8, (3, 4)), (12, 8, 3, 0, 7, (3, 5)), (13, 2, 2, BIG // 169 + 3, 4, (1, 2)), (3, 16, 2, 2, 6, (2, 3))):
        n = 2 * R
        s = qu.random_boards(N, n, 70 + N, over=True)
        seeds = abi.seeds_for(1000 * N, n)
        betas, ladder = np.linspace(0.3, 1.5, total), ladder_of(R, 0.5, 2.0)
        rungs = permuted_rungs(n, R, N)
        whole = tempering.temper_states_host(N, s, seeds, betas, ladder, exchange_every=K, first_sweep=first, rungs=rungs, trace=True)
        followed = set()
        for cut in cuts:
            followed.add((first + cut) % K == 0)
            a = tempering.temper_states_host(N, s, seeds, betas[:cut], ladder, exchange_every=K, first_sweep=first, rungs=rungs, trace=True)
            b = tempering.temper_states_host(N, a["state"], seeds, betas[cut:], ladder, exchange_every=K, first_sweep=first + cut, rungs=a["rung_out"], trace=True)
            what = f"N={N} R={R} K={K} cut at {cut} of {total}"
            for k in ("state", "energy_out", "rung_out"):
                np.testing.assert_array_equal(b[k], whole[k], err_msg=f"{what}: {k}")
            np.testing.assert_array_equal(b["energy_in"], a["energy_out"], err_msg=what)
            for k in ("energy_hist", "rung_hist"):
                np.testing.assert_array_equal(np.concatenate([a[k], b[k][:, 1:]], axis=1), whole[k], err_msg=f"{what}: {k}")
            for k in ("n_changed", "n_exchanges", "pair_accepted"):
                np.testing.assert_array_equal(a[k] + b[k], whole[k], err_msg=f"{what}: {k}")
            later = b["best_energy"] < a["best_energy"]
            np.testing.assert_array_equal(np.where(later, b["best_energy"], a["best_energy"]), whole["best_energy"], err_msg=what)
            np.testing.assert_array_equal(np.where(later, b["best_sweep"] + cut, a["best_sweep"]), whole["best_sweep"], err_msg=what)
            np.testing.assert_array_equal(np.where(later[:, None], b["best_state"], a["best_state"]), whole["best_state"], err_msg=what)
        assert followed == {True, False}, (N, followed)
        assert N == 13 or whole["n_exchanges"].sum() > 0  # (two events of one pair at N = 13: the colder slot stays lower)


def _wilson_hilferty(df, z=3.090232306167813):  # the 99.9 % quantile of chi^2 with df degrees of freedom
    return df * (1 - 2 / (9 * df) + z * np.sqrt(2 / (9 * df))) ** 3


def test_stationary_distribution_of_every_rung_is_boltzmann():
    """N = 3, 8 192 ladders of R = 4, beta = 1 with the ladder (0.5, 0.75, 1.0, 1.5), K = 1, 40 sweeps.  For each rung t the final
    energies of the slots that END on t -- one per ladder, hence independent -- against the exact Boltzmann weights of all 3^9
    placements at beta l_t.  Bins of expected count < 5 are merged; chi^2 must stay below its 99.9 % quantile, for the seed bases 42,
    100000 and 4000000000: twelve histograms.  Seeded, hence deterministic: a value above the bound is a finding, not a reseed.
    Measured, rungs 0 .. 3 (bounds 32.91, 31.26, 27.88, 24.32 at 12, 11, 9, 7 degrees of freedom): base 42: 10.36, 9.88, 5.09, 3.57;
    base 100000: 12.41, 5.77, 12.20, 3.87; base 4000000000: 8.18, 10.24, 5.01, 8.47."""
    N, L, R, T = 3, 8192, 4, 40
    ladder = (0.5, 0.75, 1.0, 1.5)
    exact = [hu.boltzmann_energy_distribution(N, 1.0 * l) for l in ladder]
    try:
        from scipy.stats import chi2

        quantile = lambda df: float(chi2.ppf(0.999, df))  # noqa: E731
    except ImportError:
        quantile = _wilson_hilferty
    failures = []
    for base in (42, 100000, 4000000000):
        s = qu.random_boards(N, L * R, base % 1000)
        got = tempering.temper_states_host(N, s, abi.seeds_for(base, L * R), [1.0] * T, ladder)
        assert got["n_exchanges"].min() >= 0 and got["pair_accepted"].sum() > L  # the ladders did exchange
        for t in range(R):
            final = got["energy_out"][got["rung_out"] == t]
            assert len(final) == L
            energies = sorted(exact[t])
            expected = np.array([exact[t][e] * L for e in energies])
            observed = np.array([int((final == e).sum()) for e in energies], dtype=np.float64)
            assert observed.sum() == L, "an energy that no placement has"
            exp_m, obs_m, ea, oa = [], [], 0.0, 0.0
            for e, o in zip(expected, observed):  # merge neighbours until every bin expects at least 5
                ea, oa = ea + e, oa + o
                if ea >= 5:
                    exp_m.append(ea), obs_m.append(oa)
                    ea = oa = 0.0
            if ea > 0:
                exp_m[-1] += ea
                obs_m[-1] += oa
            exp_m, obs_m = np.array(exp_m), np.array(obs_m)
            chi = float(((obs_m - exp_m) ** 2 / exp_m).sum())
            df = len(exp_m) - 1
            print(f"seeds {base}+ rung {t} (beta {ladder[t]}): chi^2 = {chi:.2f} with {df} degrees of freedom, bound {quantile(df):.2f}")
            if not chi < quantile(df):
                failures.append((base, t, chi, quantile(df)))
    assert not failures, failures


def test_refusals_name_the_field():
    L = mcq_amd._lib.lib()
    n, N, R, K = 8, 6, 4, 2
    buf, seeds = np.zeros((n, 36), dtype=np.uint8), np.zeros(n, dtype=np.uint32)
    T, X = abi.temper_tables([1.0, 2.0, 2.5], [0.5, 1.0, 1.5, 2.0], K, 1)
    assert X.shape[0] == 2
    hist, rhist = np.zeros((n, 4), dtype=np.int32), np.zeros((n, 4), dtype=np.uint8)
    bad_rungs = np.array([0, 1, 2, 3, 0, 1, 1, 3], dtype=np.uint8)
    high_rungs = np.array([0, 1, 2, 3, 0, 1, 2, 4], dtype=np.uint8)

    def block(**kw):
        q = tempering._block(N, n, 3, 1, R, K, T.shape[2], X.shape[2])
        q.seeds, q.table, q.swap_table = seeds.ctypes.data, T.ctypes.data, X.ctypes.data
        q.state_in = q.state_out = buf.ctypes.data
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    big = (1 << 63) // 36
    refused = ((dict(mode=abi.MODE_FULL3D), b"boards only"), (dict(N=1), b"N out of range"), (dict(N=129), b"N out of range"),
               (dict(n_chains=0), b"n_chains"), (dict(n_chains=1 << 31), b"n_chains"), (dict(replicas=3), b"2, 4, 8 or 16"),
               (dict(replicas=1), b"2, 4, 8 or 16"), (dict(replicas=32), b"2, 4, 8 or 16"), (dict(replicas=0), b"2, 4, 8 or 16"),
               (dict(replicas=16), b"must divide"), (dict(n_chains=6), b"must divide"), (dict(n_sweeps=-1), b"n_sweeps"),
               (dict(first_sweep=-1), b"first_sweep"), (dict(first_sweep=big), b"below 2^63"), (dict(exchange_every=0), b"exchange_every"),
               (dict(exchange_every=-2), b"exchange_every"), (dict(n_events=1), b"n_events"), (dict(n_events=3), b"n_events"),
               (dict(n_events=0), b"n_events"), (dict(exchange_every=1), b"n_events"), (dict(table_len=0), b"table_len"), (dict(table_len=513), b"table_len"),
               (dict(swap_len=0), b"swap_len"), (dict(swap_len=4097), b"swap_len"), (dict(seeds=None), b"seeds"), (dict(table=None), b"table is required"),
               (dict(swap_table=None), b"swap_table"), (dict(state_in=None), b"state_in"), (dict(state_out=None), b"state_out"),
               (dict(energy_hist=hist.ctypes.data, hist_stride=3), b"hist_stride"), (dict(rung_hist=rhist.ctypes.data, hist_stride=0), b"hist_stride"))
    for kw, msg in refused:
        for fn in (L.mcq_temper_host, lambda q: L.mcq_temper_device(q, None)):  # the device entry point refuses before any launch: no GPU here
            assert fn(ctypes.byref(block(**kw))) == abi.EINVAL, kw
            assert msg in L.mcq_temper_last_error(), (kw, L.mcq_temper_last_error())
    assert L.mcq_temper_host(None) == abi.EINVAL and L.mcq_temper_device(None, None) == abi.EINVAL
    assert L.mcq_temper_host(ctypes.byref(block())) == abi.OK
    assert L.mcq_temper_host(ctypes.byref(block(energy_hist=hist.ctypes.data, rung_hist=rhist.ctypes.data, hist_stride=4))) == abi.OK
    assert L.mcq_temper_host(ctypes.byref(block(hist_stride=-5))) == abi.OK  # read only when a history is asked for
    assert L.mcq_temper_host(ctypes.byref(block(n_sweeps=0, n_events=0, table=None, swap_table=None))) == abi.OK  # first_sweep = 1: no event
    # N = 2: 2^61 events times 16 replicas would wrap the exchange stream's word index
    wide = np.zeros((16, 4), dtype=np.uint8)
    q = block(N=2, n_chains=16, replicas=16, first_sweep=(1 << 61) - 8, n_sweeps=0, exchange_every=1, n_events=0, state_in=wide.ctypes.data, state_out=wide.ctypes.data)
    assert L.mcq_temper_host(ctypes.byref(q)) == abi.EINVAL and b"exchange stream" in L.mcq_temper_last_error()
    # the host code reads its inputs: the rungs and the table
    for rungs in (bad_rungs, high_rungs):
        assert L.mcq_temper_host(ctypes.byref(block(rung_in=rungs.ctypes.data))) == abi.EINVAL
        assert b"no permutation" in L.mcq_temper_last_error() and b"ladder 1" in L.mcq_temper_last_error()
    over = T.copy()
    over[1, 2, 0] = (1 << 24) + 1
    assert L.mcq_temper_host(ctypes.byref(block(table=over.ctypes.data))) == abi.EINVAL
    assert b"sweep 1, rung 2" in L.mcq_temper_last_error() and b"above 2^24" in L.mcq_temper_last_error()
    before = buf.copy()
    assert L.mcq_temper_host(ctypes.byref(block(n_events=5))) == abi.EINVAL and (buf == before).all()  # before any work
    # the LDS limit of the device entry point, without a GPU: the message names N, R and the bytes
    for Nn, Rr, nbytes in ((64, 8, 8 * 6 * 64 * 64 + 8 * 4 * T.shape[2] + 96), (64, 16, None), (65, 2, None), (128, 2, None), (33, 8, None)):
        st = np.zeros((16, Nn * Nn), dtype=np.uint8)
        sd = np.zeros(16, dtype=np.uint32)
        q = block(N=Nn, n_chains=16, replicas=Rr, seeds=sd.ctypes.data, state_in=st.ctypes.data, state_out=st.ctypes.data)
        assert L.mcq_temper_device(ctypes.byref(q), None) == abi.EINVAL, (Nn, Rr)
        msg = L.mcq_temper_last_error()
        assert f"N = {Nn} with replicas = {Rr}".encode() in msg and b"bytes of LDS" in msg, msg
        if nbytes:
            assert f"takes {nbytes} bytes".encode() in msg, msg
    assert L.mcq_temper_host(ctypes.byref(block(table_len=0))) == abi.EINVAL and L.mcq_heatbath_host(None) == abi.EINVAL
    assert b"table_len" in L.mcq_temper_last_error()  # its own message: the heat bath's refusal left it alone


def test_temper_struct_layout_and_build():
    fields = [f for f, _ in abi.Temper._fields_]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "mcq.h"\nint main(){printf("%zu %d %d %d", sizeof(mcq_temper), MCQ_ABI_VERSION, ' \
        'MCQ_MAX_TEMPER_SWAP_TABLE, MCQ_MAX_TEMPER_LDS);' + "".join(f'printf(" %zu", offsetof(mcq_temper, {f}));' for f in fields) + "return 0;}"
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(prog)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")], check=True)
        out = subprocess.run([os.path.join(d, "t")], capture_output=True, text=True, check=True).stdout.split()
    assert int(out[0]) == ctypes.sizeof(abi.Temper) and int(out[1]) == 6 == abi.ABI_VERSION
    assert int(out[2]) == abi.MAX_TEMPER_SWAP_TABLE == 4096 and int(out[3]) == abi.MAX_TEMPER_LDS == 160 * 1024
    assert [int(x) for x in out[4:]] == [getattr(abi.Temper, f).offset for f in fields]
    assert set(abi.TEMPER_DTYPES) < set(fields) and set(abi.HEATBATH_DTYPES) < set(abi.TEMPER_DTYPES)
    L = mcq_amd._lib.lib()
    assert L.mcq_abi_version() == 6
    built = mcq_amd.build.TEMPER_SOURCES
    assert built == [os.path.join(mcq_amd.build.CSRC, "mcq_temper.hip")] and all(os.path.exists(f) for f in built)
    assert len(mcq_amd.build.SOURCES) == 6 and len(mcq_amd.build.ADDED_SOURCES) == 1
    for name in ("mcq_temper_device", "mcq_temper_host", "mcq_temper_last_error"):
        assert hasattr(L, name), name
    for name in ("temper_states", "temper_device", "temper_states_host", "anneal_tempered"):
        assert callable(getattr(tempering, name)), name
    t = os.path.getmtime(mcq_amd.build.SO)
    assert all(os.path.getmtime(f) <= t for f in built) or mcq_amd.build.stale()  # stale() watches the new list
