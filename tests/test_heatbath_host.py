"""CPU-only: the heat-bath rule in host code (mcq_heatbath_host) against its NumPy restatement (tests/heatbath_util.py) on every output,
the restatement's own ingredients against the oracle's Philox and the reference's conflict counts, the properties of the rule, its
stationary distribution on a board small enough to enumerate, every refusal, and the layout of the mcq_heatbath block."""
import ctypes
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

import mcq_amd
from tests import heatbath_util as hu
from tests import quench_util as qu

abi = mcq_amd.abi
heatbath = mcq_amd.heatbath
quench = mcq_amd.quench
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restatement_philox_equals_the_oracles():
    from oracle import oracle

    rs = np.random.RandomState(5)
    for _ in range(40):
        ctr = [int(rs.randint(0, 2**32, dtype=np.uint64)), int(rs.randint(1, 2**31, dtype=np.uint64)), 0, 0]  # a non-zero high word
        key = [int(rs.randint(0, 2**32, dtype=np.uint64)), 1]
        assert hu.philox(ctr, key) == [int(x) for x in oracle.philox_block(ctr, key)], (ctr, key)
    for ctr, key in (([0, 0, 0, 0], [0, 1]), ([2**32 - 1, 2**32 - 1, 0, 0], [2**32 - 1, 1]), ([1, 2, 3, 4], [5, 6])):
        assert hu.philox(ctr, key) == [int(x) for x in oracle.philox_block(ctr, key)], (ctr, key)
    # word w of the stream: block w / 4 split into two counter words, element w % 4, key word 1
    w = (3 << 34) + 4 * 77 + 2
    assert hu.word(9, w) == int(oracle.philox_block([77, 3, 0, 0], [9, 1])[2])
    assert hu.word(9, w) != int(oracle.philox_block([77, 3, 0, 0], [9, 0])[2])  # not the sweep's Philox stream


def test_restatement_counts_are_the_references():
    z = np.load(os.path.join(ROOT, "tests", "golden", "conflicts.npz"))
    cases = json.loads(str(z["cases"]))
    assert len(cases) >= 28
    for c in cases:
        N, key = c["N"], c["key"]
        h = qu.clamp(N, z[key + "_heights"])
        want = z[key + "_table"].astype(np.int64)
        for col in range(N * N) if N <= 17 else range(0, N * N, 7):
            np.testing.assert_array_equal(qu.column(N, h, col), want[col], err_msg=f"{c['what']} column {col}")


def test_table_builder():
    for betas in ([0.0], [3.0], [1.0, 2.0, 3.0], [0.01, 0.02], [0.5] * 4, [40.0], [0.0, 3.0], []):
        got, want = abi.heatbath_table(betas), hu.table(betas)
        assert got.dtype == np.uint32 and got.flags.c_contiguous
        np.testing.assert_array_equal(got, want, err_msg=str(betas))
        assert (got[:, 0] == 1 << 24).all() and 1 <= got.shape[1] <= 512
    assert abi.heatbath_table([0.0]).shape == (1, 512) and (abi.heatbath_table([0.0]) == 1 << 24).all()
    t = abi.heatbath_table([1.0, 3.0])
    assert t.shape[1] == 18 and t[0, 16] == 1 and t[0, 17] == 0 and t[1, 6] == 0 and t[1, 5] > 0  # floor(2^24 e^-16) = 1, e^-17 -> 0
    assert abi.heatbath_table([40.0]).shape == (1, 2)
    for bad in ([-0.1], [1.0, float("nan")], [float("inf")]):
        with pytest.raises(ValueError, match="beta >= 0"):
            abi.heatbath_table(bad)


# (N, chains, betas, first_sweep)
CASES = [(N, 3 if N <= 12 else 2, [(0.0, 3.0, 1.0), (0.5, 0.5), (3.0,), (1.0, 2.0)][N % 4], [0, 3, (1 << 34) // (N * N) + 5][N % 3]) for N in range(2, 25)] + \
        [(31, 1, (0.7,), 2), (32, 2, (3.0,), 0), (33, 1, (0.0,), 1 << 40), (64, 1, (1.5,), 0), (65, 1, (0.3,), 9), (127, 1, (2.0,), 0), (128, 1, (0.004,), 1)]


def test_host_code_equals_the_restatement():
    total = 0
    for idx, (N, n, betas, first) in enumerate(CASES):
        s = qu.random_boards(N, n, 4000 + idx, over=idx % 3 == 1)
        if idx % 4 == 0:
            s[0] = idx % N
        if idx % 5 == 0:
            s[-1] = 255  # every byte clamped to N - 1
        seeds = [(977 * idx + 31 * r) % 2**32 for r in range(n)]
        seeds[-1] = 2**32 - 1 - idx
        what = f"N={N} betas={betas} first_sweep={first} ({n} boards)"
        want = hu.sweeps_many(N, s, seeds, betas, first)
        got = heatbath.heatbath_states_host(N, s, seeds, betas, first_sweep=first, trace=True)
        hu.assert_equal(got, want, what, hist=True)
        assert got["state"].dtype == np.uint8 and got["best_sweep"].dtype == np.int64 and got["n_changed"].dtype == np.int64
        assert got["energy_in"].dtype == np.int32 and int(got["state"].max()) < N
        plain = heatbath.heatbath_states_host(N, s, seeds, betas, first_sweep=first)  # history off
        assert "energy_hist" not in plain
        hu.assert_equal(plain, want, what + " without the history")
        # in place, only the placements and the energy: state_out = state_in, every other output optional
        buf, e_out = s.copy(), np.zeros(n, dtype=np.int32)
        tab, sd = abi.heatbath_table(betas), np.array(seeds, dtype=np.uint32)
        q = abi.Heatbath()
        q.N, q.mode, q.n_chains, q.n_sweeps, q.first_sweep, q.table_len = N, abi.MODE_BOARD, n, len(betas), first, tab.shape[1]
        q.seeds, q.table, q.energy_out = sd.ctypes.data, tab.ctypes.data, e_out.ctypes.data
        q.state_in = q.state_out = buf.ctypes.data
        mcq_amd._lib.heatbath_host(q)
        np.testing.assert_array_equal(buf, want["state"], err_msg=what + ": in place")
        np.testing.assert_array_equal(e_out, want["energy_out"], err_msg=what + ": in place")
        total += n
    assert total >= 50
    assert abi.heatbath_table((0.004,)).shape[1] == 512  # the N = 128 case runs with the table capped at D = 512


def test_no_sweep_is_a_recount_and_a_copy():
    for N in (2, 7, 12, 33):
        s = qu.random_boards(N, 4, N, over=True)
        got = heatbath.heatbath_states_host(N, s, [1, 2, 3, 4], [], first_sweep=11, trace=True)
        clamped = np.minimum(s, N - 1)
        np.testing.assert_array_equal(got["state"], clamped)
        np.testing.assert_array_equal(got["best_state"], clamped)
        want = quench.quench_states_host(N, s, max_passes=1)["energy_in"]
        for k in ("energy_in", "energy_out", "best_energy"):
            np.testing.assert_array_equal(got[k], want, err_msg=k)
        assert not got["best_sweep"].any() and not got["n_changed"].any() and got["energy_hist"].shape == (4, 1)
        np.testing.assert_array_equal(got["energy_hist"][:, 0], want)
        # ... with no table at all
        q = abi.Heatbath()
        out, sd = np.zeros_like(s), np.zeros(4, dtype=np.uint32)
        q.N, q.mode, q.n_chains, q.table_len, q.seeds, q.state_in, q.state_out = N, abi.MODE_BOARD, 4, 1, sd.ctypes.data, s.ctypes.data, out.ctypes.data
        mcq_amd._lib.heatbath_host(q)
        np.testing.assert_array_equal(out, clamped)


def test_segments_with_first_sweep_carried_equal_one_call():
    for N, n, cut, total, first in ((6, 5, 2, 5, 0), (12, 3, 1, 4, 7), (13, 2, 3, 4, (1 << 35) // 169), (20, 2, 2, 3, 100)):
        betas = np.linspace(0.5, 3.0, total)
        s = qu.random_boards(N, n, 50 + N, over=True)
        seeds = np.arange(n) + 1000 * N
        whole = heatbath.heatbath_states_host(N, s, seeds, betas, first_sweep=first, trace=True)
        a = heatbath.heatbath_states_host(N, s, seeds, betas[:cut], first_sweep=first, trace=True)
        b = heatbath.heatbath_states_host(N, a["state"], seeds, betas[cut:], first_sweep=first + cut, trace=True)
        what = f"N={N} cut at {cut} of {total}"
        np.testing.assert_array_equal(b["state"], whole["state"], err_msg=what)
        np.testing.assert_array_equal(b["energy_out"], whole["energy_out"], err_msg=what)
        np.testing.assert_array_equal(b["energy_in"], a["energy_out"], err_msg=what)
        np.testing.assert_array_equal(a["energy_in"], whole["energy_in"], err_msg=what)
        np.testing.assert_array_equal(np.concatenate([a["energy_hist"], b["energy_hist"][:, 1:]], axis=1), whole["energy_hist"], err_msg=what)
        np.testing.assert_array_equal(a["n_changed"] + b["n_changed"], whole["n_changed"], err_msg=what)
        # the merge rule of chains in segments: a later segment moves the best only by a strictly lower energy
        later = b["best_energy"] < a["best_energy"]
        np.testing.assert_array_equal(np.where(later, b["best_energy"], a["best_energy"]), whole["best_energy"], err_msg=what)
        np.testing.assert_array_equal(np.where(later, b["best_sweep"] + cut, a["best_sweep"]), whole["best_sweep"], err_msg=what)
        np.testing.assert_array_equal(np.where(later[:, None], b["best_state"], a["best_state"]), whole["best_state"], err_msg=what)
        other = heatbath.heatbath_states_host(N, s, seeds, betas, first_sweep=first + 1)
        assert (other["state"] != whole["state"]).any(), "first_sweep does not move the stream"


def test_invariants_on_random_cases():
    rs = np.random.RandomState(99)
    for idx, N in enumerate((2, 3, 4, 6, 9, 12, 15, 16, 17, 24, 40)):
        n, T = (6, 5) if N <= 17 else (2, 2)
        betas = rs.uniform(0.0, 3.0, size=T)
        s = qu.random_boards(N, n, 300 + idx, over=idx % 2 == 0)
        seeds = rs.randint(0, 2**32, size=n, dtype=np.uint64)
        got = heatbath.heatbath_states_host(N, s, seeds, betas, first_sweep=idx, trace=True)
        hist = got["energy_hist"]
        recount = lambda states: quench.quench_states_host(N, states, max_passes=1, conflicts=False)["energy_in"]  # noqa: E731
        np.testing.assert_array_equal(got["energy_out"], recount(got["state"]), err_msg=f"N={N}: energy_out is not the energy of state_out")
        np.testing.assert_array_equal(got["energy_in"], recount(s))
        np.testing.assert_array_equal(hist[:, 0], got["energy_in"])
        np.testing.assert_array_equal(hist[:, -1], got["energy_out"])
        np.testing.assert_array_equal(got["best_energy"], hist.min(axis=1))
        np.testing.assert_array_equal(got["best_sweep"], hist.argmin(axis=1))  # the FIRST index of the minimum
        np.testing.assert_array_equal(recount(got["best_state"]), got["best_energy"])
        assert (got["n_changed"] >= 0).all() and (got["n_changed"] <= T * N * N).all()
        for r in range(n):
            if got["best_sweep"][r] == T:
                np.testing.assert_array_equal(got["best_state"][r], got["state"][r])


def test_a_table_of_one_entry_makes_every_update_uniform():
    """D = 1: every height has the weight T[0], so k = floor(x N / 2^32) whatever the placement."""
    for N in (2, 5, 12, 16, 33, 100):
        Q = N * N
        seeds = np.array([17, 4000000000], dtype=np.uint32)
        tab = np.full((2, 1), 1 << 24, dtype=np.uint32)
        for first in (0, 3, (1 << 34) // Q + 1):
            outs = []
            for boards in (qu.random_boards(N, 2, N + first % 7, over=True), np.zeros((2, Q), dtype=np.uint8)):
                q = abi.Heatbath()
                out = np.zeros_like(boards)
                q.N, q.mode, q.n_chains, q.n_sweeps, q.first_sweep, q.table_len = N, abi.MODE_BOARD, 2, 2, first, 1
                q.seeds, q.table, q.state_in, q.state_out = seeds.ctypes.data, tab.ctypes.data, boards.ctypes.data, out.ctypes.data
                mcq_amd._lib.heatbath_host(q)
                outs.append(out)
            np.testing.assert_array_equal(outs[0], outs[1], err_msg=f"N={N}: the placement mattered")
            cols = range(Q) if N <= 16 else range(0, Q, 37)
            for r in range(2):
                want = [(hu.word(int(seeds[r]), (first + 1) * Q + c) * N) >> 32 for c in cols]  # the second sweep's words are what is left
                assert [int(outs[0][r][c]) for c in cols] == want, (N, first, r)


def _wilson_hilferty(df, z=3.090232306167813):  # the 99.9 % quantile of chi^2 with df degrees of freedom
    return df * (1 - 2 / (9 * df) + z * np.sqrt(2 / (9 * df))) ** 3


@pytest.mark.parametrize("beta", (0.5, 1.0))
def test_stationary_distribution_is_boltzmann(beta):
    """N = 3: the histogram of the final energies of 8 192 chains after 40 sweeps at constant beta against the exact Boltzmann weights
    of all 3^9 placements.  Bins of expected count < 5 are merged; chi^2 must stay below its 99.9 % quantile.  Seeded, hence
    deterministic: a failure is a finding about the rule or its implementation."""
    N, n, T = 3, 8192, 40
    exact = hu.boltzmann_energy_distribution(N, beta)
    assert abs(sum(exact.values()) - 1) < 1e-12
    boards, E = hu.all_placements(N)
    for r in np.random.RandomState(1).randint(0, len(E), size=25):  # the enumeration's energies are the rule's
        assert qu.energy(N, boards[r]) == int(E[r])
    try:
        from scipy.stats import chi2

        quantile = lambda df: float(chi2.ppf(0.999, df))  # noqa: E731
    except ImportError:
        quantile = _wilson_hilferty
    for base in (42, 100000, 4000000000):
        s = qu.random_boards(N, n, base % 1000)
        got = heatbath.heatbath_states_host(N, s, abi.seeds_for(base, n), [beta] * T)
        energies = sorted(exact)
        expected = np.array([exact[e] * n for e in energies])
        observed = np.array([int((got["energy_out"] == e).sum()) for e in energies], dtype=np.float64)
        assert observed.sum() == n, "an energy that no placement has"
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
        print(f"beta={beta} seeds {base}+: chi^2 = {chi:.2f} with {df} degrees of freedom, bound {quantile(df):.2f}")
        assert chi < quantile(df), f"beta={beta}, seeds {base}+: chi^2 = {chi:.2f} >= {quantile(df):.2f} ({df} degrees of freedom)"


def test_refusals_name_the_field():
    L = mcq_amd._lib.lib()
    buf, seeds, tab = np.zeros((4, 36), dtype=np.uint8), np.zeros(4, dtype=np.uint32), abi.heatbath_table([1.0, 2.0])
    hist = np.zeros((4, 3), dtype=np.int32)

    def block(**kw):
        q = abi.Heatbath()
        q.N, q.mode, q.n_chains, q.n_sweeps, q.first_sweep, q.table_len = 6, abi.MODE_BOARD, 4, 2, 0, tab.shape[1]
        q.seeds, q.table = seeds.ctypes.data, tab.ctypes.data
        q.state_in = q.state_out = buf.ctypes.data
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    big = (1 << 63) // 36
    refused = ((dict(mode=abi.MODE_FULL3D), b"boards only"), (dict(mode=7), b"mode"), (dict(N=1), b"N out of range"), (dict(N=129), b"N out of range"),
               (dict(n_chains=0), b"n_chains"), (dict(n_chains=-1), b"n_chains"), (dict(n_chains=1 << 31), b"n_chains"),
               (dict(n_sweeps=-1), b"n_sweeps"), (dict(first_sweep=-1), b"first_sweep"), (dict(first_sweep=big), b"below 2^63"),
               (dict(first_sweep=big - 1), b"below 2^63"), (dict(first_sweep=(1 << 63) - 1), b"below 2^63"),
               (dict(table_len=0), b"table_len"), (dict(table_len=513), b"table_len"), (dict(seeds=None), b"seeds"), (dict(table=None), b"table"),
               (dict(state_in=None), b"state_in"), (dict(state_out=None), b"state_out"),
               (dict(energy_hist=hist.ctypes.data, hist_stride=2), b"hist_stride"), (dict(energy_hist=hist.ctypes.data, hist_stride=0), b"hist_stride"))
    for kw, msg in refused:
        for fn in (L.mcq_heatbath_host, lambda q: L.mcq_heatbath_device(q, None)):  # the device entry point refuses before any launch: no GPU here
            assert fn(ctypes.byref(block(**kw))) == abi.EINVAL, kw
            assert msg in L.mcq_heatbath_last_error(), (kw, L.mcq_heatbath_last_error())
    assert L.mcq_heatbath_host(None) == abi.EINVAL and L.mcq_heatbath_device(None, None) == abi.EINVAL
    assert L.mcq_heatbath_host(ctypes.byref(block())) == abi.OK
    assert L.mcq_heatbath_host(ctypes.byref(block(first_sweep=big - 2))) == abi.OK  # (big - 2 + 2) 36 < 2^63 still
    assert L.mcq_heatbath_host(ctypes.byref(block(energy_hist=hist.ctypes.data, hist_stride=3))) == abi.OK
    assert L.mcq_heatbath_host(ctypes.byref(block(hist_stride=-5))) == abi.OK  # read only when a history is asked for
    assert L.mcq_heatbath_host(ctypes.byref(block(table_len=0))) == abi.EINVAL and L.mcq_quench_host(None) == abi.EINVAL
    assert b"table_len" in L.mcq_heatbath_last_error()  # its own message: the quench's refusal left it alone
    with pytest.raises(ValueError, match="N out of range"):
        heatbath.heatbath_states_host(200, np.zeros((2, 40000), dtype=np.uint8), [1, 2], [1.0])
    with pytest.raises(ValueError, match="first_sweep"):
        heatbath.heatbath_states_host(6, buf, seeds, [1.0], first_sweep=-2)
    with pytest.raises(ValueError, match="n_chains"):
        heatbath.heatbath_states_host(6, np.zeros((0, 36), dtype=np.uint8), [], [1.0])
    with pytest.raises(ValueError, match="final_state layout"):
        heatbath.heatbath_states_host(6, np.zeros((2, 35), dtype=np.uint8), [1, 2], [1.0])
    with pytest.raises(ValueError, match="one entry per chain"):
        heatbath.heatbath_states_host(6, buf, [1, 2], [1.0])
    with pytest.raises(ValueError, match="Seed must be"):
        heatbath.heatbath_states_host(6, buf, [1, 2, 3, -1], [1.0])
    with pytest.raises(ValueError, match="beta >= 0"):
        heatbath.heatbath_states_host(6, buf, seeds, [1.0, -1.0])


def test_anneal_heatbath_refuses_before_anything_is_launched():
    """None of these reaches the GPU: there is none here."""
    lin = {"type": "linear_annealing", "beta_start": 1.0, "beta_end": 3.0}
    down = {"type": "linear_annealing", "beta_start": 3.0, "beta_end": 1.0}
    boards = qu.random_boards(6, 64, 1)
    seeds = abi.seeds_for(42, 64)
    run = heatbath.anneal_heatbath
    with pytest.raises(ValueError, match="does not decrease"):
        run(6, 100, boards, down, seeds, resample_every=10)
    with pytest.raises(ValueError, match="resample_every must be positive"):
        run(6, 100, boards, lin, seeds, resample_every=0)
    with pytest.raises(ValueError, match="must divide"):
        run(6, 100, boards, lin, seeds, resample_every=10, population=48)
    with pytest.raises(ValueError, match="multiple of 16"):
        run(6, 100, boards, lin, seeds, resample_every=10, population=8)
    with pytest.raises(ValueError, match="multiple of 16"):
        run(6, 100, boards, lin, abi.seeds_for(0, 40), resample_every=10)
    with pytest.raises(ValueError, match="at most 2\\^19"):
        heatbath.check(1 << 20, 100, 10)
    with pytest.raises(ValueError, match="at least one sweep"):
        run(6, 0, boards, lin, seeds, resample_every=10)
    with pytest.raises(ValueError, match="n_sweeps"):
        run(6, -1, boards, lin, seeds)
    with pytest.raises(ValueError, match="beta >= 0"):
        run(6, 10, boards, {"type": "constant", "beta_const": -1.0}, seeds)
    with pytest.raises(ValueError, match="one schedule"):
        run(6, 10, boards, [lin, lin], seeds)
    with pytest.raises(ValueError, match="N out of range"):
        run(129, 10, "random", lin, seeds)
    with pytest.raises(ValueError, match="one placement per seed"):
        run(6, 10, boards[:32], lin, seeds)
    with pytest.raises(ValueError, match="Unknown init_mode"):
        run(6, 10, "diagonal", lin, seeds)
    assert heatbath.check(256, 100, 7, 64) == (7, 64) and heatbath.check(256, 100, 7) == (7, 256)


def test_heatbath_struct_layout_and_build():
    fields = [f for f, _ in abi.Heatbath._fields_]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "mcq.h"\nint main(){printf("%zu %d %d", sizeof(mcq_heatbath), MCQ_ABI_VERSION, MCQ_MAX_HEATBATH_TABLE);' + \
        "".join(f'printf(" %zu", offsetof(mcq_heatbath, {f}));' for f in fields) + "return 0;}"
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(prog)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")], check=True)
        out = subprocess.run([os.path.join(d, "t")], capture_output=True, text=True, check=True).stdout.split()
    assert int(out[0]) == ctypes.sizeof(abi.Heatbath) and int(out[1]) == 6 == abi.ABI_VERSION and int(out[2]) == abi.MAX_HEATBATH_TABLE == 512
    assert [int(x) for x in out[3:]] == [getattr(abi.Heatbath, f).offset for f in fields]
    assert fields == ["N", "mode", "n_chains", "n_sweeps", "first_sweep", "seeds", "table", "table_len", "state_in", "state_out", "energy_in",
                      "energy_out", "best_energy", "best_sweep", "best_state", "n_changed", "energy_hist", "hist_stride"]
    L = mcq_amd._lib.lib()
    assert os.path.join(mcq_amd.build.CSRC, "mcq_heatbath.hip") in mcq_amd.build.SOURCES
    for name in ("mcq_heatbath_device", "mcq_heatbath_host", "mcq_heatbath_last_error"):
        assert hasattr(L, name), name
    assert mcq_amd.heatbath.anneal_heatbath and "heatbath_sweeps" in mcq_amd.drivers.run_competition.__code__.co_varnames
