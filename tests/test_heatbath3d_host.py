"""CPU-only: the full_3d heat-bath rule in host code (mcq_heatbath3d_host) against its NumPy restatement (tests/heatbath3d_util.py) on
every output, the consequences of the rule (a table of one entry, a zero-temperature table, segments, no sweep, repeated cells), every
refusal, the layout of the mcq_heatbath3d block, and the stationary distribution of the sweep on a cube small enough to enumerate."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

import mcq_amd
from tests import heatbath3d_util as h3
from tests import heatbath_util as hu
from tests import quench3d_util as q3
from tests.heatbath_tables_util import host3d as _raw

abi = mcq_amd.abi
heatbath = mcq_amd.heatbath
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_philox_words_with_key_word_two_are_the_oracles():
    from oracle import oracle

    rs = np.random.RandomState(6)
    for _ in range(20):
        ctr = [int(rs.randint(0, 2**32, dtype=np.uint64)), int(rs.randint(1, 2**30, dtype=np.uint64)), 0, 0]
        seed = int(rs.randint(0, 2**32, dtype=np.uint64))
        assert hu.philox(ctr, (seed, 2)) == [int(x) for x in oracle.philox_block(ctr, [seed, 2])], (ctr, seed)
    # update u takes the words 2 u and 2 u + 1: both in block u / 2, elements 0, 1 for an even u and 2, 3 for an odd one
    u = (5 << 33) + 2 * 91
    blk = [int(x) for x in oracle.philox_block([91, 5, 0, 0], [9, 2])]
    assert h3.draw(9, u) == blk[0] | blk[1] << 32 and h3.draw(9, u + 1) == blk[2] | blk[3] << 32
    assert h3.word(9, 2 * u) != hu.word(9, 2 * u) and h3.word(9, 2 * u) != int(oracle.philox_block([91, 5, 0, 0], [9, 0])[0])  # its own stream
    c = h3._philox_many([91, 7], [5, 0], [9, 9], [2, 2])
    assert [int(v[0]) for v in c] == blk and [int(v[1]) for v in c] == [int(x) for x in oracle.philox_block([7, 0, 0, 0], [9, 2])]


# (N, Q or None = N^2, chains, betas, over)
CASES = [(N, None, 4 if N <= 5 else 2, [0.7, 0.0, 3.0] if N <= 6 else [0.0, 1.5], N % 3 == 1) for N in range(2, 9)] + \
        [(12, 144, 2, [0.0], False), (13, 40, 2, [0.7, 0.0], True), (19, 45, 2, [0.0, 2.0], False), (20, 45, 2, [1.0], True), (32, 24, 2, [0.0], False),
         (2, 2, 4, [0.0, 1.0, 20.0], False), (2, 7, 3, [0.5, 0.0], True), (2, 4, 3, [2.0], False),
         (3, 2, 3, [0.0, 1.0], False), (3, 26, 3, [0.3, 20.0], False), (3, 13, 3, [1.0], True),
         (4, 2, 2, [0.0], False), (4, 63, 2, [0.0, 1.0], True), (4, 30, 2, [20.0, 0.1], False),
         (5, 2, 2, [1.0], False), (5, 124, 2, [0.0, 0.7], False), (5, 60, 2, [3.0], True),
         (7, 49, 2, [20.0, 20.0], False), (9, 30, 2, [0.05, 40.0], False)]


def test_host_code_equals_the_restatement():
    total, big, two = 0, 0, 0
    for idx, (N, Q, n, betas, over) in enumerate(CASES):
        Qn = N * N if Q is None else Q
        s = q3.random_placements(N, n, 5000 + idx, Q=Q, over=over)
        seeds = abi.seeds_for(100 + idx, n)
        first = (0, 3, (1 << 40) + 1)[idx % 3]
        want_rows = [h3.sweeps(N, s[r], int(seeds[r]), hu.table(betas), len(betas), first) for r in range(n)]
        want = {k: np.stack([np.asarray(r[k]) for r in want_rows]) for k in h3.FIELDS + ("energy_hist",)}
        got = heatbath.heatbath_queens_host(N, s, seeds, betas, Q=Q, first_sweep=first, trace=True)
        what = f"N={N} Q={Qn} betas={betas} first_sweep={first}"
        h3.assert_equal(got, want, what, hist=True)
        assert set(got) == set(heatbath.FIELDS_3D) | {"energy_hist"} and set(heatbath.FIELDS_3D) == set(heatbath.FIELDS) | {"flags"}
        assert got["state"].dtype == np.uint8 and got["best_sweep"].dtype == np.int64 and got["n_changed"].dtype == np.int64
        assert got["state"].shape == (n, 3 * Qn) and int(got["state"].max()) < N and not got["flags"].any()
        h3.assert_equal(heatbath.heatbath_queens_host(N, s.reshape(n, Qn, 3), seeds, betas, Q=Q, first_sweep=first), want, what + " as [n][Q][3]")
        big += sum(1 for r in want_rows for d in r["draws"] if d[2] > 1 << 32)
        if min(betas) == 20.0:
            assert hu.table(betas).shape[1] == 2  # D = 2
            two += 1
        # in place, and no optional output
        buf = s.copy()
        q = abi.Heatbath3D()
        tab = abi.heatbath_table(betas)
        q.N, q.n_queens, q.n_chains, q.n_sweeps, q.first_sweep, q.table_len = N, 0 if Q is None else Q, n, len(betas), first, tab.shape[1]
        q.seeds, q.table = seeds.ctypes.data, tab.ctypes.data
        q.state_in = q.state_out = buf.ctypes.data
        mcq_amd._lib.heatbath3d_host(q)
        np.testing.assert_array_equal(buf, want["state"], err_msg=f"{what}: in place")
        total += n
    assert total >= 60 and two >= 1 and big >= 100  # W beyond 32 bits: the beta = 0 rows from N = 7 on


def test_a_table_of_one_entry_makes_every_update_uniform():
    """D = 1: every candidate has the weight T[0], so the new cell is the floor(x F / 2^64)-th free cell, whatever the placement."""
    for idx, (N, Q) in enumerate(((2, 2), (2, 7), (3, 9), (4, 16), (5, 100), (7, 49), (13, 30), (20, 10))):
        n, n_sweeps, first = 2, 2, (0, 11)[idx % 2]
        s = q3.random_placements(N, n, 600 + idx, Q=Q)
        seeds = abi.seeds_for(7 + idx, n)
        for t0 in (1 << 24, 12345):
            got = _raw(N, Q, s, seeds, np.full((n_sweeps, 1), t0, dtype=np.uint32), n_sweeps, first)
            F = N ** 3 - Q + 1
            for r in range(n):
                z = q3.clamp(N, s[r]).copy()
                for sw in range(n_sweeps):
                    for q in range(Q):
                        idx_all = h3.cell_index(N, z)
                        free = np.setdiff1d(np.arange(N ** 3), np.delete(idx_all, q))
                        assert len(free) == F
                        t = int(free[(h3.draw(int(seeds[r]), (first + sw) * Q + q) * F) >> 64])
                        z[q] = q3._cells(N)[t]
                np.testing.assert_array_equal(got["state"][r], z.astype(np.uint8).reshape(-1), err_msg=f"N={N} Q={Q} chain {r}")
                assert int(got["energy_out"][r]) == q3.energy(N, z)


def test_a_zero_temperature_table_never_raises_the_energy():
    """T = [2^24, 0]: only the cells of the minimal count carry weight, and the queen's own cell is a candidate."""
    tab1 = np.array([[1 << 24, 0]], dtype=np.uint32)
    for idx, (N, Q) in enumerate(((3, 9), (4, 16), (6, 36), (8, 64), (12, 144), (13, 60), (20, 80))):
        n, n_sweeps = 3, 3
        s = q3.random_placements(N, n, 900 + idx, Q=Q)
        got = _raw(N, Q, s, abi.seeds_for(idx, n), np.repeat(tab1, n_sweeps, axis=0), n_sweeps)
        h = got["energy_hist"]
        assert (np.diff(h, axis=1) <= 0).all() and (h[:, -1] < h[:, 0]).all(), (N, Q, h)
        np.testing.assert_array_equal(got["best_energy"], h.min(axis=1))
        same = heatbath.heatbath_queens_host(N, s, abi.seeds_for(idx, n), [20.0] * n_sweeps, Q=Q, trace=True)  # floor(2^24 e^-20) = 0
        h3.assert_equal(same, got, f"N={N}: beta = 20 builds that table", hist=True)


def test_consistency_of_segments_recount_and_outputs():
    for idx, (N, Q, n) in enumerate(((2, None, 4), (3, None, 4), (4, 40, 3), (6, None, 4), (8, 30, 3), (12, None, 2), (13, 50, 2), (20, 60, 2), (32, 40, 1))):
        Qn = N * N if Q is None else Q
        s = q3.random_placements(N, n, 1200 + idx, Q=Q, over=idx % 2 == 0)
        seeds = abi.seeds_for(55 + idx, n)
        betas = [0.2, 0.6, 1.0, 1.4, 3.0][: 5 if N <= 13 else 3]
        what = f"N={N} Q={Qn}"
        whole = heatbath.heatbath_queens_host(N, s, seeds, betas, Q=Q, first_sweep=7, trace=True)
        # the output is a placement of distinct cells with the energy the updates added up
        for r in range(n):
            assert not q3.is_repeated(N, whole["state"][r]) and not q3.is_repeated(N, whole["best_state"][r]), what
            assert q3.energy(N, whole["state"][r]) == int(whole["energy_out"][r]) == int(whole["energy_hist"][r, -1]), what
            assert q3.energy(N, whole["best_state"][r]) == int(whole["best_energy"][r]), what
            assert q3.energy(N, s[r]) == int(whole["energy_in"][r]) == int(whole["energy_hist"][r, 0]), what
        assert ((0 <= whole["n_changed"]) & (whole["n_changed"] <= len(betas) * Qn)).all()
        bs = whole["best_sweep"]
        np.testing.assert_array_equal(whole["energy_hist"][np.arange(n), bs], whole["best_energy"])
        np.testing.assert_array_equal(whole["energy_hist"].min(axis=1), whole["best_energy"])
        np.testing.assert_array_equal(whole["energy_hist"].argmin(axis=1), bs)  # the FIRST sweep end with the minimum
        # segments with first_sweep carried over
        cut = 2
        a = heatbath.heatbath_queens_host(N, s, seeds, betas[:cut], Q=Q, first_sweep=7, trace=True)
        b = heatbath.heatbath_queens_host(N, a["state"], seeds, betas[cut:], Q=Q, first_sweep=7 + cut, trace=True)
        np.testing.assert_array_equal(b["state"], whole["state"], err_msg=what)
        np.testing.assert_array_equal(b["energy_in"], a["energy_out"])
        np.testing.assert_array_equal(np.concatenate([a["energy_hist"], b["energy_hist"][:, 1:]], axis=1), whole["energy_hist"])
        np.testing.assert_array_equal(a["n_changed"] + b["n_changed"], whole["n_changed"])
        np.testing.assert_array_equal(np.minimum(a["best_energy"], b["best_energy"]), whole["best_energy"])
        wrong = heatbath.heatbath_queens_host(N, a["state"], seeds, betas[cut:], Q=Q, first_sweep=0)
        assert not np.array_equal(wrong["state"], whole["state"]), f"{what}: first_sweep moves the stream"
        # no sweep: a recount and a copy (of the clamped input)
        none = heatbath.heatbath_queens_host(N, s, seeds, [], Q=Q, trace=True)
        np.testing.assert_array_equal(none["state"], np.minimum(s, N - 1))
        np.testing.assert_array_equal(none["best_state"], np.minimum(s, N - 1))
        np.testing.assert_array_equal(none["energy_in"], whole["energy_in"])
        np.testing.assert_array_equal(none["energy_out"], whole["energy_in"])
        np.testing.assert_array_equal(none["best_energy"], whole["energy_in"])
        assert none["energy_hist"].shape == (n, 1) and not none["best_sweep"].any() and not none["n_changed"].any() and not none["flags"].any()


def test_repeated_cells_are_flagged_and_nothing_moves():
    for idx, (N, Q) in enumerate(((2, 2), (3, None), (6, 20), (12, None), (19, 50), (20, 50), (5, 124))):
        Qn = N * N if Q is None else Q
        s = q3.random_placements(N, 3, 3000 + idx, Q=Q).reshape(3, Qn, 3)
        s[0, Qn - 1] = s[0, 0]  # two queens in one cell
        s[1, :, :] = 255  # every byte clamped: all queens in the corner cell
        seeds = abi.seeds_for(idx, 3)
        got = heatbath.heatbath_queens_host(N, s, seeds, [0.5, 1.0], Q=Q, trace=True)
        h3.assert_equal(got, h3.sweeps_many(N, s, seeds, [0.5, 1.0], Q=Q), f"N={N} Q={Qn}", hist=True)
        assert list(got["flags"]) == [abi.HEATBATH3D_REPEATED, abi.HEATBATH3D_REPEATED, 0]
        for r in (0, 1):
            e = q3.energy(N, s[r])
            assert int(got["energy_in"][r]) == int(got["energy_out"][r]) == int(got["best_energy"][r]) == e
            assert list(got["energy_hist"][r]) == [e, e, e] and int(got["best_sweep"][r]) == 0 == int(got["n_changed"][r])
            np.testing.assert_array_equal(got["state"][r], np.minimum(s[r], N - 1).reshape(-1))
            np.testing.assert_array_equal(got["best_state"][r], np.minimum(s[r], N - 1).reshape(-1))
        assert int(got["energy_in"][1]) == Qn * (Qn - 1) // 2
        alone = heatbath.heatbath_queens_host(N, s[2:], seeds[2:], [0.5, 1.0], Q=Q)
        for k in heatbath.FIELDS_3D:
            np.testing.assert_array_equal(alone[k][0], got[k][2], err_msg=k)


def test_refusals_name_the_field():
    L = mcq_amd._lib.lib()
    buf = np.zeros((4, 3 * 215), dtype=np.uint8)
    sd = np.arange(4, dtype=np.uint32)
    tab = abi.heatbath_table([1.0, 2.0])
    hist = np.zeros((4, 3), dtype=np.int32)

    def block(**kw):
        q = abi.Heatbath3D()
        q.N, q.n_queens, q.n_chains, q.n_sweeps, q.first_sweep, q.table_len = 6, 0, 4, 2, 0, tab.shape[1]
        q.seeds, q.table = sd.ctypes.data, tab.ctypes.data
        q.state_in = q.state_out = buf.ctypes.data
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    refused = ((dict(N=1), b"N out of range [2, 32]"), (dict(N=-3), b"N out of range"), (dict(N=33), b"stops at N = 32"), (dict(N=64), b"stops at N = 32"),
               (dict(N=65), b"N out of range [2, 32]"), (dict(n_queens=1), b"n_queens"), (dict(n_queens=-2), b"n_queens"), (dict(n_queens=216), b"N^3 - 1 = 215"),
               (dict(n_chains=0), b"n_chains"), (dict(n_chains=-1), b"n_chains"), (dict(n_chains=1 << 31), b"n_chains"),
               (dict(n_sweeps=-1), b"n_sweeps"), (dict(first_sweep=-1), b"first_sweep"), (dict(first_sweep=(1 << 62) // 36 - 1), b"below 2^62"),
               (dict(first_sweep=1 << 61, n_queens=2), b"below 2^62"), (dict(table_len=0), b"table_len"), (dict(table_len=513), b"table_len"),
               (dict(seeds=None), b"seeds"), (dict(table=None), b"table is required"), (dict(state_in=None), b"state_in"), (dict(state_out=None), b"state_out"),
               (dict(energy_hist=hist.ctypes.data, hist_stride=2), b"hist_stride"))
    for kw, msg in refused:
        for fn in (L.mcq_heatbath3d_host, lambda q: L.mcq_heatbath3d_device(q, None)):  # the device entry point refuses before any launch: no GPU here
            assert fn(ctypes.byref(block(**kw))) == abi.EINVAL, kw
            assert msg in L.mcq_heatbath3d_last_error(), (kw, L.mcq_heatbath3d_last_error())
    assert L.mcq_heatbath3d_host(None) == abi.EINVAL and L.mcq_heatbath3d_device(None, None) == abi.EINVAL
    assert b"NULL" in L.mcq_heatbath3d_last_error()
    assert L.mcq_heatbath3d_host(ctypes.byref(block())) == abi.OK
    assert L.mcq_heatbath3d_host(ctypes.byref(block(first_sweep=(1 << 62) // 36 - 3))) == abi.OK  # (first_sweep + 2) 36 < 2^62
    assert L.mcq_heatbath3d_host(ctypes.byref(block(table=None, n_sweeps=0))) == abi.OK
    assert L.mcq_heatbath3d_host(ctypes.byref(block(energy_hist=hist.ctypes.data, hist_stride=3))) == abi.OK
    # a message of its own: the board heat-bath's is untouched by these calls, and it still refuses full_3d
    hb = abi.Heatbath()
    hb.N, hb.mode, hb.n_chains, hb.n_sweeps, hb.table_len = 6, abi.MODE_FULL3D, 4, 2, tab.shape[1]
    hb.seeds, hb.table, hb.state_in, hb.state_out = sd.ctypes.data, tab.ctypes.data, buf.ctypes.data, buf.ctypes.data
    assert L.mcq_heatbath_host(ctypes.byref(hb)) == abi.EINVAL and b"boards only" in L.mcq_heatbath_last_error()
    L.mcq_heatbath3d_host(ctypes.byref(block(N=40)))
    assert b"boards only" in L.mcq_heatbath_last_error() and b"stops at N = 32" in L.mcq_heatbath3d_last_error()
    s6 = np.zeros((2, 108), dtype=np.uint8)
    with pytest.raises(ValueError, match="N out of range"):
        heatbath.heatbath_queens_host(40, np.zeros((2, 4800), dtype=np.uint8), [1, 2], [1.0])
    with pytest.raises(ValueError, match="first_sweep"):
        heatbath.heatbath_queens_host(6, s6, [1, 2], [1.0], first_sweep=-1)
    with pytest.raises(ValueError, match="n_chains"):
        heatbath.heatbath_queens_host(6, np.zeros((0, 108), dtype=np.uint8), [], [1.0])
    with pytest.raises(ValueError, match="n_queens"):
        heatbath.heatbath_queens_host(3, np.zeros((2, 81), dtype=np.uint8), [1, 2], [1.0], Q=27)
    with pytest.raises(ValueError, match="final_state layout of full_3d"):
        heatbath.heatbath_queens_host(6, np.zeros((2, 107), dtype=np.uint8), [1, 2], [1.0])
    with pytest.raises(ValueError, match="beta >= 0"):
        heatbath.heatbath_queens_host(6, s6, [1, 2], [-1.0])
    with pytest.raises(ValueError, match="one entry per chain"):
        heatbath.heatbath_queens_host(6, s6, [1, 2, 3], [1.0])
    # anneal_heatbath's new keywords, before anything is launched
    lin = {"type": "linear_annealing", "beta_start": 1.0, "beta_end": 3.0}
    run = heatbath.anneal_heatbath
    with pytest.raises(ValueError, match="Unknown mcmc_type"):
        run(6, 10, "random", lin, abi.seeds_for(1, 64), mcmc_type="cube")
    with pytest.raises(ValueError, match="N out of range \\[2, 32\\]"):
        run(33, 10, "random", lin, abi.seeds_for(1, 64), mcmc_type="full_3d")
    with pytest.raises(ValueError, match="n_queens"):
        run(3, 10, "random", lin, abi.seeds_for(1, 64), mcmc_type="full_3d", Q=27)
    with pytest.raises(ValueError, match="a board has one height per column"):
        run(6, 10, "random", lin, abi.seeds_for(1, 64), Q=30)
    with pytest.raises(ValueError, match="one placement per seed"):
        run(6, 10, np.zeros((32, 108), dtype=np.uint8), lin, abi.seeds_for(1, 64), mcmc_type="full_3d")
    with pytest.raises(ValueError, match="multiple of 16"):
        run(6, 100, np.zeros((64, 108), dtype=np.uint8), lin, abi.seeds_for(1, 64), resample_every=10, population=8, mcmc_type="full_3d")


def test_heatbath3d_struct_layout_and_build():
    fields = [f for f, _ in abi.Heatbath3D._fields_]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "mcq.h"\nint main(){printf("%zu %d %d %d", sizeof(mcq_heatbath3d), MCQ_ABI_VERSION, ' \
        'MCQ_MAX_HEATBATH_TABLE, MCQ_HEATBATH3D_REPEATED);' + "".join(f'printf(" %zu", offsetof(mcq_heatbath3d, {f}));' for f in fields) + "return 0;}"
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(prog)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")], check=True)
        out = subprocess.run([os.path.join(d, "t")], capture_output=True, text=True, check=True).stdout.split()
    assert int(out[0]) == ctypes.sizeof(abi.Heatbath3D) and int(out[1]) == 6 == abi.ABI_VERSION
    assert int(out[2]) == abi.MAX_HEATBATH_TABLE == 512 and int(out[3]) == abi.HEATBATH3D_REPEATED == 1
    assert [int(x) for x in out[4:]] == [getattr(abi.Heatbath3D, f).offset for f in fields]
    hb = [f for f, _ in abi.Heatbath._fields_]
    assert fields == [("n_queens" if f == "mode" else f) for f in hb] + ["flags"]  # the board block with n_queens for mode, and flags
    assert set(abi.HEATBATH3D_DTYPES) < set(fields)
    L = mcq_amd._lib.lib()
    built = mcq_amd.build.SOURCES + mcq_amd.build.ADDED_SOURCES
    assert os.path.join(mcq_amd.build.CSRC, "mcq_heatbath3d.hip") in built and len(built) == 7 and all(os.path.exists(f) for f in built)
    for name in ("mcq_heatbath3d_device", "mcq_heatbath3d_host", "mcq_heatbath3d_last_error"):
        assert hasattr(L, name), name
    for name in ("heatbath_queens", "heatbath_queens_device", "heatbath_queens_host"):
        assert callable(getattr(heatbath, name)), name


def _stationary_start(n, seed):
    rs = np.random.RandomState(seed)
    flat = np.stack([rs.choice(27, size=3, replace=False) for _ in range(n)])
    return np.stack([flat // 9, (flat // 3) % 3, flat % 3], axis=2).astype(np.uint8).reshape(n, 9)


@pytest.mark.parametrize("beta", [0.5, 1.0])
def test_stationary_distribution_is_boltzmann(beta):
    """N = 3, Q = 3: all 17 550 ordered placements of distinct cells are enumerated (E = 0 .. 3); 8 192 chains from random distinct
    placements run 40 sweeps at constant beta, and the histogram of their final energies is compared with the exact Boltzmann shares:
    chi^2 over the four levels below 16.27, the 99.9 % quantile at 3 degrees of freedom, for three fixed seed bases.  (A float NumPy
    simulation of the rule gave 0.7 .. 3.7.)  The restatement passes the same test."""
    n, n_sweeps = 8192, 40
    count, shares = h3.boltzmann_energy_shares(3, 3, beta)
    assert count == 17550 and sorted(shares) == [0, 1, 2, 3] and abs(sum(shares.values()) - 1.0) < 1e-12
    assert min(shares.values()) * n >= 379  # no level needs merging
    tab = hu.table([beta] * n_sweeps)
    for base in (11, 2024, 777777):
        start, seeds = _stationary_start(n, base), abi.seeds_for(base, n)
        got = heatbath.heatbath_queens_host(3, start, seeds, [beta] * n_sweeps, Q=3)
        x2 = h3.chi2(got["energy_out"], shares)
        state, E = h3.sweeps_batch(3, start, seeds, tab, n_sweeps)
        x2r = h3.chi2(E, shares)
        print(f"beta={beta} seed base {base}: chi^2 = {x2:.2f} (host code), {x2r:.2f} (restatement)")
        assert x2 < 16.27 and x2r < 16.27, (beta, base, x2, x2r)
        np.testing.assert_array_equal(state, got["state"])  # and the two are the same chains
        assert not got["flags"].any()
