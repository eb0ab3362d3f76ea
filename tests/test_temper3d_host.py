"""CPU-only: the full_3d tempering rule in host code (mcq_temper3d_host) against its NumPy restatement (tests/temper3d_util.py) on every
output, against the plain full_3d heat-bath host code where the two must agree, the invariants of the exchange, segments, the held
ladder, the stationary distribution of every rung on a cube small enough to enumerate, every refusal -- the LDS limit of the device entry
point among them --, and the layout of the mcq_temper3d block."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

import mcq_amd
from tests import heatbath3d_util as h3
from tests import quench3d_util as q3
from tests import temper3d_util as t3

abi = mcq_amd.abi
heatbath = mcq_amd.heatbath
tempering = mcq_amd.tempering
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = 1 << 34
HB3 = heatbath.FIELDS_3D + ("energy_hist",)


def ladder_of(R, lo=0.5, hi=1.5):
    return [float(x) for x in np.linspace(lo, hi, R)]


def permuted_rungs(n, R, seed):
    rs = np.random.RandomState(seed)
    return np.concatenate([rs.permutation(R) for _ in range(n // R)]).astype(np.uint8)


# (N, Q or None = N^2, R, ladders, K, first_sweep, sweeps, rung_in given)
CASES = [(2, None, 16, 2, 1, 0, 6, False), (2, 2, 4, 2, 3, BIG // 2 + 2, 7, True), (2, 7, 2, 3, 2, 3, 5, True),
         (3, None, 4, 2, 2, 3, 4, True), (3, 2, 16, 1, 1, BIG // 2 + 1, 3, False), (3, 26, 2, 2, 3, 4, 5, False),
         (4, None, 2, 2, 1, BIG // 16 + 5, 3, True), (4, 63, 4, 1, 2, 1, 3, False), (4, 2, 16, 1, 3, 2, 6, True),
         (5, None, 4, 1, 2, 1, 3, True), (5, 124, 2, 1, 1, 0, 2, False), (5, 2, 16, 1, 2, 5, 4, False), (3, None, 2, 1, 1, 7, 0, True)]


def test_host_code_equals_the_restatement():
    taken = refused = 0
    seen = set()
    for idx, (N, Q, R, ladders, K, first, T, given) in enumerate(CASES):
        n, Qn = R * ladders, N * N if Q is None else Q
        assert K == 1 or first % K or T == 0, "first_sweep off a multiple of K"
        s = q3.random_placements(N, n, 7000 + idx, Q=Q, over=idx % 2 == 0)  # (over: bytes >= N that clamp back to N - 1)
        seeds = [(1237 * idx + 77 * r) % 2**32 for r in range(n)]
        seeds[0] = 2**32 - 1 - idx
        betas = list(np.linspace(0.2, 1.2, T))
        ladder = ladder_of(R, 0.5, 2.0)
        rungs = permuted_rungs(n, R, idx) if given else None
        what = f"N={N} Q={Qn} R={R} K={K} first_sweep={first} sweeps={T} rung_in={'given' if given else 'default'}"
        want = t3.run_many(N, s, seeds, betas, ladder, Q, K, first, rungs)
        got = tempering.temper_queens_host(N, s, seeds, betas, ladder, Q=Q, exchange_every=K, first_sweep=first, rungs=rungs, trace=True)
        t3.assert_equal(got, want, what, hist=True)
        assert set(got) == set(tempering.FIELDS_3D) | {"energy_hist", "rung_hist"} and set(tempering.FIELDS_3D) == set(tempering.FIELDS) | {"flags"}
        assert got["rung_out"].dtype == got["rung_hist"].dtype == np.uint8 and got["n_exchanges"].dtype == got["pair_accepted"].dtype == np.int64
        assert got["flags"].dtype == np.int32 and not got["flags"].any()
        assert got["pair_accepted"].shape == (ladders, R - 1) and got["state"].shape == (n, 3 * Qn) and int(got["state"].max()) < N
        plain = tempering.temper_queens_host(N, s.reshape(n, Qn, 3), seeds, betas, ladder, Q=Q, exchange_every=K, first_sweep=first, rungs=rungs)
        assert "energy_hist" not in plain and "rung_hist" not in plain
        t3.assert_equal(plain, want, what + " as [n][Q][3], without the histories")
        for draws in want["draws"]:
            for e, t, delta, x, swap in draws:
                seen.add((N, R, K))
                taken += x is not None and swap
                refused += x is not None and not swap
    print(f"pairs decided by the table: {taken} swapped, {refused} did not")
    assert taken >= 5 and refused >= 5, (taken, refused)  # the table decided both ways
    assert {c[0] for c in seen} == {2, 3, 4, 5} and {c[1] for c in seen} == {2, 4, 16} and {c[2] for c in seen} == {1, 2, 3}


def test_equal_multipliers_are_plain_heatbath_chains():
    """R equal rows: every heatbath.FIELDS_3D output is heatbath_queens_host's with the same seeds and betas, whatever the exchanges do."""
    for N, Q, R, K, first in ((3, None, 4, 1, 0), (6, 20, 16, 2, 3), (8, None, 2, 1, 5), (13, 30, 8, 3, 1)):
        n = 2 * R
        s = q3.random_placements(N, n, N, Q=Q, over=True)
        seeds = abi.seeds_for(500 + N, n)
        betas = np.linspace(0.5, 2.0, 4)
        got = tempering.temper_queens_host(N, s, seeds, betas, [0.75] * R, Q=Q, exchange_every=K, first_sweep=first, trace=True)
        want = heatbath.heatbath_queens_host(N, s, seeds, betas * 0.75, Q=Q, first_sweep=first, trace=True)
        for k in HB3:
            np.testing.assert_array_equal(got[k], want[k], err_msg=f"N={N} R={R}: {k}")
        assert got["n_exchanges"].sum() > 0  # and the rungs did move


def test_without_an_event_each_slot_follows_its_own_rung():
    for N, Q, R in ((3, None, 4), (5, 40, 16), (9, None, 2)):
        n, T = 2 * R, 3
        s = q3.random_placements(N, n, 11 * N, Q=Q)
        seeds = abi.seeds_for(9, n)
        betas, ladder = np.array([0.4, 1.0, 1.6]), ladder_of(R)
        rungs = permuted_rungs(n, R, N)
        got = tempering.temper_queens_host(N, s, seeds, betas, ladder, Q=Q, exchange_every=T + 1, rungs=rungs, trace=True)
        assert not got["n_exchanges"].any() and not got["pair_accepted"].any() and (got["rung_hist"] == rungs[:, None]).all()
        np.testing.assert_array_equal(got["rung_out"], rungs)
        for r in range(n):
            want = heatbath.heatbath_queens_host(N, s[r: r + 1], seeds[r: r + 1], betas * ladder[rungs[r]], Q=Q, trace=True)
            for k in HB3:
                np.testing.assert_array_equal(got[k][r: r + 1], want[k], err_msg=f"N={N} slot {r}: {k}")


def test_invariants_on_random_cases():
    rs = np.random.RandomState(123)
    for idx, (N, Q, R) in enumerate(((2, None, 16), (3, 5, 4), (4, None, 8), (5, 60, 2), (8, None, 16), (13, 40, 4), (20, 30, 8))):
        K, first, T = 1 + idx % 3, int(rs.randint(0, 9)), 8
        n = R * (6 if N <= 5 else 2)
        s = q3.random_placements(N, n, 900 + idx, Q=Q, over=idx % 2 == 1)
        seeds = rs.randint(0, 2**32, size=n, dtype=np.uint64)
        betas = rs.uniform(0.1, 1.5, size=T)
        rungs = permuted_rungs(n, R, idx) if idx % 2 else None
        ladder = ladder_of(R, 0.4, 2.0)
        got = tempering.temper_queens_host(N, s, seeds, betas, ladder, Q=Q, exchange_every=K, first_sweep=first, rungs=rungs, trace=True)
        t3.check_invariants(got, R, K, first)
        recount = mcq_amd.quench.quench_queens_host(N, got["state"], Q=Q, max_passes=1, conflicts=False)["energy_in"]
        np.testing.assert_array_equal(got["energy_out"], recount)
        np.testing.assert_array_equal(got["best_energy"], got["energy_hist"].min(axis=1))
        np.testing.assert_array_equal(got["best_sweep"], got["energy_hist"].argmin(axis=1))
        # a swap table of zeros: x < 0 never holds, so a pair swaps exactly when Delta >= 0
        Tt, X = abi.temper_tables(betas, ladder, K, first)
        Xz = np.zeros_like(X) if X.size else np.zeros((1, R - 1, 1), dtype=np.uint32)
        zero = t3.host_call(N, N * N if Q is None else Q, s, seeds, Tt, Xz, K, first, rungs)
        t3.check_invariants(zero, R, K, first, swap_zero=True)


def test_the_pairs_word_is_the_one_the_rule_names():
    """Key word 4, the seed of the ladder's slot 0, word e R + t: recomputed here with the oracle's Philox, and the decision with it."""
    from oracle import oracle
    from tests import temper_util as tu

    N, Q, R, K, first, T = 4, 16, 4, 2, 5, 12
    n = 3 * R
    s = q3.random_placements(N, n, 31, Q=Q)
    seeds = np.array([(4000000000 + 17 * r) % 2**32 for r in range(n)], dtype=np.uint32)
    betas, ladder = np.full(T, 0.6), [0.5, 1.0, 1.5, 2.0]
    Tt, X = abi.temper_tables(betas, ladder, K, first)
    got = tempering.temper_queens_host(N, s, seeds, betas, ladder, Q=Q, exchange_every=K, first_sweep=first, trace=True)
    rh, eh = got["rung_hist"].astype(int).reshape(3, R, -1), got["energy_hist"].astype(int).reshape(3, R, -1)
    looked = other = 0
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
                x = int(oracle.philox_block([(w >> 2) & 0xFFFFFFFF, w >> 34, 0, 0], [int(seeds[g * R]), 4])[w & 3])
                assert x == t3.exchange_word(int(seeds[g * R]), w) and x != tu.exchange_word(int(seeds[g * R]), w)  # not the boards' stream
                limit = int(X[j, t, min(-delta, X.shape[2] - 1)])
                assert swapped == (x < limit), (g, sw, t)
                other += (tu.exchange_word(int(seeds[g * R]), w) < limit) != swapped
                looked += 1
    assert looked >= 10 and other >= 1, (looked, other)  # key word 3 would have decided at least one pair the other way


def test_segments_equal_the_unbroken_call():
    """Cut at a sweep that is followed by an event and at one that is not: first_sweep, the rungs and the placements carried over, the
    swap table's rows split where the cut falls."""
    for N, Q, R, K, first, total, cuts in ((3, None, 4, 2, 1, 8, (3, 4)), (5, 30, 16, 3, 0, 7, (3, 5)), (8, None, 2, 2, BIG // 64 + 3, 4, (1, 2)), (2, 5, 16, 2, 2, 6, (2, 3))):
        n = 2 * R
        s = q3.random_placements(N, n, 70 + N, Q=Q, over=True)
        seeds = abi.seeds_for(1000 * N, n)
        betas, ladder = np.linspace(0.3, 1.5, total), ladder_of(R, 0.5, 2.0)
        rungs = permuted_rungs(n, R, N)
        kw = dict(Q=Q, exchange_every=K, trace=True)
        whole = tempering.temper_queens_host(N, s, seeds, betas, ladder, first_sweep=first, rungs=rungs, **kw)
        followed = set()
        for cut in cuts:
            followed.add((first + cut) % K == 0)
            a = tempering.temper_queens_host(N, s, seeds, betas[:cut], ladder, first_sweep=first, rungs=rungs, **kw)
            b = tempering.temper_queens_host(N, a["state"], seeds, betas[cut:], ladder, first_sweep=first + cut, rungs=a["rung_out"], **kw)
            what = f"N={N} R={R} K={K} cut at {cut} of {total}"
            for k in ("state", "energy_out", "rung_out", "flags"):
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
        assert N == 8 or whole["n_exchanges"].sum() > 0  # (two events of one pair at N = 8: the colder slot stays lower)


def test_a_repeated_slot_holds_its_whole_ladder():
    """Rule item 4: ladder 1 of three holds a repeat in slot 2 (two queens in one cell) and, in another run, one that only clamping makes."""
    for N, Q, R, clamped in ((4, None, 4, False), (3, 5, 2, True), (5, 30, 16, False)):
        Qn = N * N if Q is None else Q
        n, T, K, first = 3 * R, 4, 2, 1
        s = q3.random_placements(N, n, 40 + N, Q=Q)
        bad = R + min(2, R - 1)
        if clamped:
            s[bad, :3], s[bad, 3:6] = (N - 1, 0, 0), (200, 0, 0)  # distinct bytes, one cell after clamping
        else:
            s[bad, 3:6] = s[bad, :3]
        seeds = abi.seeds_for(77, n)
        betas, ladder = np.linspace(0.4, 1.2, T), ladder_of(R, 0.5, 2.0)
        rungs = permuted_rungs(n, R, 5)
        got = tempering.temper_queens_host(N, s, seeds, betas, ladder, Q=Q, exchange_every=K, first_sweep=first, rungs=rungs, trace=True)
        t3.assert_equal(got, t3.run_many(N, s, seeds, betas, ladder, Q, K, first, rungs), f"N={N} R={R}: a held ladder among three", hist=True)
        held = slice(R, 2 * R)
        flags = got["flags"].reshape(3, R)
        assert (flags[0] == 0).all() and (flags[2] == 0).all()
        want_flags = np.full(R, abi.TEMPER3D_HELD)
        want_flags[bad - R] = abi.TEMPER3D_HELD | abi.HEATBATH3D_REPEATED
        np.testing.assert_array_equal(flags[1], want_flags)
        assert abi.TEMPER3D_HELD == 2 and abi.HEATBATH3D_REPEATED == 1 and flags[1, bad - R] == 3
        clampd = np.minimum(s[held], N - 1)
        np.testing.assert_array_equal(got["state"][held], clampd)
        np.testing.assert_array_equal(got["best_state"][held], clampd)
        recount = np.array([q3.pairwise_energy(N, p) for p in s[held]])
        for k in ("energy_in", "energy_out", "best_energy"):
            np.testing.assert_array_equal(got[k][held], recount, err_msg=k)
        for k in ("best_sweep", "n_changed", "n_exchanges"):
            assert not got[k][held].any(), k
        np.testing.assert_array_equal(got["rung_out"][held], rungs[held])
        assert (got["energy_hist"][held] == recount[:, None]).all() and (got["rung_hist"][held] == rungs[held, None]).all()
        assert not got["pair_accepted"][1].any()
        # the neighbours ran: they are the same ladders in a call of their own (a ladder depends on its own slots and seeds only)
        for g in (0, 2):
            own = slice(g * R, (g + 1) * R)
            alone = tempering.temper_queens_host(N, s[own], seeds[own], betas, ladder, Q=Q, exchange_every=K, first_sweep=first, rungs=rungs[own], trace=True)
            for k in t3.PER_SLOT + ("energy_hist", "rung_hist"):
                np.testing.assert_array_equal(got[k][own], alone[k], err_msg=f"ladder {g}: {k}")
            np.testing.assert_array_equal(got["pair_accepted"][g], alone["pair_accepted"][0])
            assert got["n_changed"][own].all()


def _wilson_hilferty(df, z=3.090232306167813):  # the 99.9 % quantile of chi^2 with df degrees of freedom
    return df * (1 - 2 / (9 * df) + z * np.sqrt(2 / (9 * df))) ** 3


def _distinct_starts(n, seed):
    rs = np.random.RandomState(seed)
    flat = np.stack([rs.choice(27, size=3, replace=False) for _ in range(n)])
    return np.stack([flat // 9, (flat // 3) % 3, flat % 3], axis=2).astype(np.uint8).reshape(n, 9)


def test_stationary_distribution_of_every_rung_is_boltzmann():
    """N = 3, Q = 3, 8 192 ladders of R = 4 from distinct random placements, beta = 1 with the ladder (0.5, 0.75, 1.0, 1.5), K = 1, 40
    sweeps.  For each rung t the final energies of the slots that END on t -- one per ladder, hence independent -- against the exact
    Boltzmann shares of all 17 550 ordered placements at beta l_t (heatbath3d_util.boltzmann_energy_shares).  Bins of expected count
    < 5 are merged; chi^2 must stay below its 99.9 % quantile, for the seed bases 42, 100000 and 4000000000: twelve histograms.  Seeded,
    hence deterministic: a value above the bound is a finding, not a reseed.
    Measured, rungs 0 .. 3 (bound 16.27 at 3 degrees of freedom each): base 42: 3.44, 1.06, 0.30, 3.63; base 100000: 3.74, 4.38, 0.81,
    2.63; base 4000000000: 3.78, 0.54, 2.12, 0.79."""
    N, Q, L, R, T = 3, 3, 8192, 4, 40
    ladder = (0.5, 0.75, 1.0, 1.5)
    exact = [h3.boltzmann_energy_shares(N, Q, 1.0 * l)[1] for l in ladder]
    try:
        from scipy.stats import chi2

        quantile = lambda df: float(chi2.ppf(0.999, df))  # noqa: E731
    except ImportError:
        quantile = _wilson_hilferty
    failures = []
    for base in (42, 100000, 4000000000):
        s = _distinct_starts(L * R, base % 1000)
        got = tempering.temper_queens_host(N, s, abi.seeds_for(base, L * R), [1.0] * T, ladder, Q=Q)
        assert not got["flags"].any() and got["pair_accepted"].sum() > L  # the ladders did exchange
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
    n, N, R, K = 8, 4, 4, 2
    buf, seeds = np.zeros((n, 3 * 63), dtype=np.uint8), np.zeros(n, dtype=np.uint32)
    buf[:, :48] = np.tile(q3.random_placements(N, 1, 1)[0], (n, 1))
    T, X = abi.temper_tables([1.0, 2.0, 2.5], [0.5, 1.0, 1.5, 2.0], K, 1)
    assert X.shape[0] == 2
    hist, rhist = np.zeros((n, 4), dtype=np.int32), np.zeros((n, 4), dtype=np.uint8)
    bad_rungs = np.array([0, 1, 2, 3, 0, 1, 1, 3], dtype=np.uint8)
    high_rungs = np.array([0, 1, 2, 3, 0, 1, 2, 4], dtype=np.uint8)

    def block(**kw):
        q = tempering._block3d(N, 0, n, 3, 1, R, K, T.shape[2], X.shape[2])
        q.seeds, q.table, q.swap_table = seeds.ctypes.data, T.ctypes.data, X.ctypes.data
        q.state_in = q.state_out = buf.ctypes.data
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    refused = ((dict(N=1), b"N out of range [2, 32]"), (dict(N=-3), b"N out of range"), (dict(N=33), b"stops at N = 32"), (dict(N=64), b"stops at N = 32"),
               (dict(N=65), b"N out of range [2, 32]"), (dict(n_queens=1), b"n_queens"), (dict(n_queens=-2), b"n_queens"), (dict(n_queens=64), b"N^3 - 1 = 63"),
               (dict(n_chains=0), b"n_chains"), (dict(n_chains=1 << 31), b"n_chains"), (dict(replicas=3), b"2, 4, 8 or 16"),
               (dict(replicas=1), b"2, 4, 8 or 16"), (dict(replicas=32), b"2, 4, 8 or 16"), (dict(replicas=0), b"2, 4, 8 or 16"),
               (dict(replicas=16), b"must divide"), (dict(n_chains=6), b"must divide"), (dict(n_sweeps=-1), b"n_sweeps"),
               (dict(first_sweep=-1), b"first_sweep"), (dict(first_sweep=(1 << 62) // 16), b"below 2^62"), (dict(first_sweep=1 << 61, n_queens=2), b"below 2^62"),
               (dict(exchange_every=0), b"exchange_every"), (dict(exchange_every=-2), b"exchange_every"), (dict(n_events=1), b"n_events"),
               (dict(n_events=3), b"n_events"), (dict(n_events=0), b"n_events"), (dict(exchange_every=1), b"n_events"), (dict(table_len=0), b"table_len"),
               (dict(table_len=513), b"table_len"), (dict(swap_len=0), b"swap_len"), (dict(swap_len=4097), b"swap_len"), (dict(seeds=None), b"seeds"),
               (dict(table=None), b"table is required"), (dict(swap_table=None), b"swap_table"), (dict(state_in=None), b"state_in"),
               (dict(state_out=None), b"state_out"), (dict(energy_hist=hist.ctypes.data, hist_stride=3), b"hist_stride"),
               (dict(rung_hist=rhist.ctypes.data, hist_stride=0), b"hist_stride"))
    for kw, msg in refused:
        for fn in (L.mcq_temper3d_host, lambda q: L.mcq_temper3d_device(q, None)):  # the device entry point refuses before any launch: no GPU here
            assert fn(ctypes.byref(block(**kw))) == abi.EINVAL, kw
            assert msg in L.mcq_temper3d_last_error(), (kw, L.mcq_temper3d_last_error())
    assert L.mcq_temper3d_host(None) == abi.EINVAL and L.mcq_temper3d_device(None, None) == abi.EINVAL
    assert b"NULL" in L.mcq_temper3d_last_error()
    assert L.mcq_temper3d_host(ctypes.byref(block())) == abi.OK
    assert L.mcq_temper3d_host(ctypes.byref(block(energy_hist=hist.ctypes.data, rung_hist=rhist.ctypes.data, hist_stride=4))) == abi.OK
    assert L.mcq_temper3d_host(ctypes.byref(block(hist_stride=-5))) == abi.OK  # read only when a history is asked for
    assert L.mcq_temper3d_host(ctypes.byref(block(n_sweeps=0, n_events=0, table=None, swap_table=None))) == abi.OK  # first_sweep = 1: no event
    # Q = 2: 2^61 events times 16 replicas would wrap the exchange stream's word index
    wide = np.zeros((16, 6), dtype=np.uint8)
    q = block(N=2, n_queens=2, n_chains=16, replicas=16, first_sweep=(1 << 60) - 8, n_sweeps=0, exchange_every=1, n_events=0, state_in=wide.ctypes.data,
              state_out=wide.ctypes.data)
    assert L.mcq_temper3d_host(ctypes.byref(q)) == abi.EINVAL and b"exchange stream" in L.mcq_temper3d_last_error()
    # the host code reads its inputs: the rungs and the table
    for rungs in (bad_rungs, high_rungs):
        assert L.mcq_temper3d_host(ctypes.byref(block(rung_in=rungs.ctypes.data))) == abi.EINVAL
        assert b"no permutation" in L.mcq_temper3d_last_error() and b"ladder 1" in L.mcq_temper3d_last_error()
    over = T.copy()
    over[1, 2, 0] = (1 << 24) + 1
    assert L.mcq_temper3d_host(ctypes.byref(block(table=over.ctypes.data))) == abi.EINVAL
    assert b"sweep 1, rung 2" in L.mcq_temper3d_last_error() and b"above 2^24" in L.mcq_temper3d_last_error()
    before = buf.copy()
    assert L.mcq_temper3d_host(ctypes.byref(block(n_events=5))) == abi.EINVAL and (buf == before).all()  # before any work
    # a message of its own, and the board form still refuses full_3d
    tb = tempering._block(6, 8, 0, 0, 4, 1, 1, 1)
    tb.mode = abi.MODE_FULL3D
    assert L.mcq_temper_host(ctypes.byref(tb)) == abi.EINVAL and b"boards only" in L.mcq_temper_last_error()
    assert L.mcq_temper3d_host(ctypes.byref(block(table_len=0))) == abi.EINVAL
    assert b"boards only" in L.mcq_temper_last_error() and b"table_len" in L.mcq_temper3d_last_error()
    # Python's refusals
    s4 = q3.random_placements(4, 4, 1)
    for kw, msg in ((dict(ladder=[2.0, 1.0]), "non-decreasing"), (dict(rungs=[0, 1]), "one entry per chain"), (dict(rungs=[0, 1, 1, 1]), "no permutation"),
                    (dict(seeds=[1, 2, 3]), "one entry per chain"), (dict(betas=[-1.0]), "beta >= 0"), (dict(first_sweep=-1), "first_sweep"),
                    (dict(Q=64), "n_queens"), (dict(N=40), "N out of range"), (dict(states=s4[:, :47]), "final_state layout of full_3d"),
                    (dict(states=s4[:3], seeds=[1, 2, 3]), "must divide"), (dict(states=np.zeros((0, 48), dtype=np.uint8), seeds=[]), "n_chains")):
        a = dict(dict(N=4, states=s4, seeds=[1, 2, 3, 4], betas=[1.0], ladder=[1.0, 2.0]), **kw)
        if "Q" in kw:
            a["states"] = np.zeros((4, 192), dtype=np.uint8)
        with pytest.raises(ValueError, match=msg):
            tempering.temper_queens_host(a.pop("N"), a.pop("states"), a.pop("seeds"), a.pop("betas"), a.pop("ladder"), **a)
    lin = {"type": "linear_annealing", "beta_start": 1.0, "beta_end": 3.0}
    run = tempering.anneal_tempered  # before anything is launched
    with pytest.raises(ValueError, match="Unknown mcmc_type"):
        run(6, 10, "random", lin, abi.seeds_for(1, 8), [1.0, 2.0], mcmc_type="cube")
    with pytest.raises(ValueError, match="N out of range \\[2, 32\\]"):
        run(33, 10, "random", lin, abi.seeds_for(1, 8), [1.0, 2.0], mcmc_type="full_3d")
    with pytest.raises(ValueError, match="n_queens"):
        run(3, 10, "random", lin, abi.seeds_for(1, 8), [1.0, 2.0], mcmc_type="full_3d", Q=27)
    with pytest.raises(ValueError, match="a board has one height per column"):
        run(6, 10, "random", lin, abi.seeds_for(1, 8), [1.0, 2.0], Q=30)
    with pytest.raises(ValueError, match="must divide"):
        run(6, 10, "random", lin, abi.seeds_for(1, 7), [1.0, 2.0], mcmc_type="full_3d")
    with pytest.raises(ValueError, match="one placement per seed"):
        run(6, 10, np.zeros((4, 108), dtype=np.uint8), lin, abi.seeds_for(1, 8), [1.0, 2.0], mcmc_type="full_3d")


def _device_refuses(N, R, Q, D=512):
    """mcq_temper3d_device on a block of that shape with a NULL stream and no seeds: (refused for the LDS, the message).  Nothing is
    launched: the entry point judges the shape, then the LDS, then the buffers, so a ladder that fits stops at the missing seeds."""
    L = mcq_amd._lib.lib()
    Qn = N * N if Q is None else Q
    st = np.zeros((R, 3 * Qn), dtype=np.uint8)
    tab = np.zeros((1, R, D), dtype=np.uint32)
    q = tempering._block3d(N, Qn, R, 1, 0, R, 2, D, 1)
    q.table, q.state_in, q.state_out = tab.ctypes.data, st.ctypes.data, st.ctypes.data
    assert L.mcq_temper3d_device(ctypes.byref(q), None) == abi.EINVAL
    msg = L.mcq_temper3d_last_error()
    assert (b"bytes of LDS" in msg) != (msg == b"seeds is required"), msg
    return b"bytes of LDS" in msg, msg


def test_the_lds_limit_of_the_device_entry_point():
    """Without a GPU: the device entry point refuses exactly the (N, R) whose ladder exceeds the LDS of a workgroup, at Q = N^2 and
    D = 512 the table of include/mcq.h (R = 16 to N = 18, 8 to N = 20, 4 to N = 25, 2 to N = 32), and the message names N, R, Q and the
    bytes.  abi.temper3d_lds_bytes is the same arithmetic."""
    L = mcq_amd._lib.lib()
    largest = {}
    for R in abi.TEMPER_REPLICAS:
        for N in range(2, 33):
            fit = t3.fits(N, R)
            assert fit == (abi.temper3d_lds_bytes(N, R) <= abi.MAX_TEMPER_LDS - abi.TEMPER3D_STATIC_LDS), (N, R)
            if fit:
                largest[R] = N
    assert largest == {2: 32, 4: 25, 8: 20, 16: 18}
    assert abi.temper3d_lds_bytes(32, 2) == 148056 and abi.temper3d_lds_bytes(12, 16, 1727) == 124096 and abi.temper3d_lds_bytes(20, 8) == 161248
    for R, N in largest.items():
        for Nn in (N, N + 1):
            if Nn > 32:
                continue
            lds, msg = _device_refuses(Nn, R, None)
            assert lds == (Nn > N), (Nn, R, msg)
            if lds:
                nbytes = abi.temper3d_lds_bytes(Nn, R)
                assert f"N = {Nn} with replicas = {R} and n_queens = {Nn * Nn}".encode() in msg and f"takes {nbytes} bytes of LDS".encode() in msg, msg
    # Q and table_len count: N = 18, R = 16 fits with N^2 queens and not with 4 000; N = 20, R = 8 fits at D = 512 only just
    assert _device_refuses(18, 16, 4000)[0] and not _device_refuses(12, 16, 1727)[0] and not _device_refuses(2, 16, 7, 1)[0]
    lds, msg = _device_refuses(32, 2, 32 ** 3 - 1)
    assert lds and f"n_queens = {32 ** 3 - 1}".encode() in msg
    for N in (19, 20, 24, 32):  # what the GPU tests leave out at their sizes
        for R in abi.TEMPER_REPLICAS:
            assert _device_refuses(N, R, None)[0] == (not t3.fits(N, R)), (N, R)
    assert L.mcq_temper3d_host(None) == abi.EINVAL


def test_temper3d_struct_layout_and_build():
    fields = [f for f, _ in abi.Temper3D._fields_]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "mcq.h"\nint main(){printf("%zu %d %d %d %d %d", sizeof(mcq_temper3d), MCQ_ABI_VERSION, ' \
        'MCQ_TEMPER3D_HELD, MCQ_MAX_TEMPER_LDS, MCQ_TEMPER3D_STATIC_LDS, MCQ_HEATBATH3D_REPEATED);' + \
        "".join(f'printf(" %zu", offsetof(mcq_temper3d, {f}));' for f in fields) + "return 0;}"
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(prog)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")], check=True)
        out = subprocess.run([os.path.join(d, "t")], capture_output=True, text=True, check=True).stdout.split()
    assert int(out[0]) == ctypes.sizeof(abi.Temper3D) and int(out[1]) == 6 == abi.ABI_VERSION
    assert int(out[2]) == abi.TEMPER3D_HELD == 2 and int(out[3]) == abi.MAX_TEMPER_LDS and int(out[4]) == abi.TEMPER3D_STATIC_LDS == 256 and int(out[5]) == 1
    assert [int(x) for x in out[6:]] == [getattr(abi.Temper3D, f).offset for f in fields]
    board = [f for f, _ in abi.Temper._fields_]
    assert fields == [("n_queens" if f == "mode" else f) for f in board] + ["flags"]  # the board block with n_queens for mode, and flags
    assert abi.TEMPER3D_DTYPES == dict(abi.TEMPER_DTYPES, flags=np.int32) and set(abi.TEMPER3D_DTYPES) < set(fields)
    L = mcq_amd._lib.lib()
    assert L.mcq_abi_version() == 6
    built = mcq_amd.build.TEMPER3D_SOURCES
    assert built == [os.path.join(mcq_amd.build.CSRC, "mcq_temper3d.hip")] and all(os.path.exists(f) for f in built)
    assert len(mcq_amd.build.SOURCES) == 6 and len(mcq_amd.build.ADDED_SOURCES) == 1 and len(mcq_amd.build.TEMPER_SOURCES) == 1
    for name in ("mcq_temper3d_device", "mcq_temper3d_host", "mcq_temper3d_last_error"):
        assert hasattr(L, name), name
    for name in ("temper_queens", "temper_queens_device", "temper_queens_host", "anneal_tempered"):
        assert callable(getattr(tempering, name)), name
    t = os.path.getmtime(mcq_amd.build.SO)
    assert all(os.path.getmtime(f) <= t for f in built) or mcq_amd.build.stale()  # stale() watches the new list
