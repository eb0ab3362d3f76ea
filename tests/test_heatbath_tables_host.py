"""CPU-only: the two heat-bath host codes (mcq_heatbath3d_host, mcq_heatbath_host) against their NumPy restatements on the caller-built
weight tables of tests/heatbath_tables_util.py -- rows with T[0] = 0, a non-zero last entry, one entry, zero rows between live ones, 512
entries of 2^24 -- which abi.heatbath_table never builds; that these tables reach what they are meant to reach (W = 0 next to W > 0
inside one chain, changed cells elsewhere), counted from the restatements' own draws; and the refusal of an entry above 2^24."""
import ctypes

import numpy as np
import pytest

import mcq_amd
from tests import heatbath3d_util as h3
from tests import heatbath_tables_util as tu
from tests import heatbath_util as hu
from tests import quench3d_util as q3
from tests import quench_util as qu

abi = mcq_amd.abi
B = tu.B
N_SWEEPS, FIRST = 3, 2

# (N, Q, chains); one chain where the restatement takes seconds per chain
CASES_3D = ((2, 4, 3), (3, 9, 3), (3, 26, 2), (5, 25, 2), (5, 2, 2), (8, 64, 1), (13, 30, 1))
# where only1 / only3 give W = 0 for some updates of a chain and W > 0 for others of the SAME chain
BOTH_3D = {"only1": ((3, 9), (5, 25), (8, 64)), "only3": ((3, 9),)}


@pytest.mark.parametrize("N,Q,n", CASES_3D)
def test_full_3d_host_code_equals_the_restatement_on_every_family(N, Q, n):
    # (placements and seeds are fixed so that, counted from the restatement below, BOTH_3D holds; about 2 % of the only1 updates at
    # N = 3, Q = 9 have W = 0, so not every seed shows one)
    s = q3.random_placements(N, n, 7100 + 10 * N + Q % 10, Q=Q, over=N % 2 == 1)
    seeds = abi.seeds_for(301 + N + Q, n)
    for name, tab in tu.tables(N_SWEEPS).items():
        what = f"full_3d N={N} Q={Q} table {name}"
        rows = [h3.sweeps(N, s[r], int(seeds[r]), tab, N_SWEEPS, FIRST) for r in range(n)]
        want = {k: np.stack([np.asarray(r[k]) for r in rows]) for k in h3.FIELDS + ("energy_hist",)}
        got = tu.host3d(N, Q, s, seeds, tab, N_SWEEPS, FIRST)
        h3.assert_equal(got, want, what, hist=True)
        # what the family reaches, from the restatement's draws (x, U, W, F, t_new) alone
        zero = [sum(1 for d in r["draws"] if d[2] == 0) for r in rows]
        live = [sum(1 for d in r["draws"] if d[2] > 0) for r in rows]
        assert all(z + v == N_SWEEPS * Q for z, v in zip(zero, live)) and not want["flags"].any(), what
        if name in tu.ZERO_ROWS:
            assert live == [0] * n and not want["n_changed"].any(), what
            np.testing.assert_array_equal(want["state"], np.minimum(s, N - 1), err_msg=what)
        elif name in tu.SPARSE:
            if (N, Q) in BOTH_3D[name]:
                assert any(z > 0 and v > 0 for z, v in zip(zero, live)), f"{what}: no chain has both W = 0 and W > 0 updates: {zero} {live}"
        else:
            assert zero == ([Q] * n if name == "altzero" else [0] * n), (what, zero)  # altzero: its one zero row
            assert (want["n_changed"] > 0).all(), what
        if name == "ones":
            assert all(d[2] == d[3] == N ** 3 - Q + 1 for r in rows for d in r["draws"]), what  # W = F
        if name == "full":
            assert all(d[2] == d[3] * B for r in rows for d in r["draws"]), what  # W = F 2^24


BOARD_N = (2, 3, 5, 8, 9, 13, 17)
# where only1 gives W = 0 for some updates of a chain and W > 0 for others of the same chain (found from the restatement's words)
BOTH_BOARD = (3, 5, 8, 9, 13, 17)


def _boards(N, n, seed):
    s = qu.random_boards(N, n, seed, over=seed % 2 == 1)
    s[n - 1] = 255  # every byte clamped
    return s


@pytest.mark.parametrize("N", BOARD_N)
def test_board_host_code_equals_the_restatement_on_every_family(N):
    n = 3
    s, seeds = _boards(N, n, 40 + N), abi.seeds_for(500 + N, n)
    for name, tab in tu.tables(N_SWEEPS).items():
        what = f"board N={N} table {name}"
        rows = [hu.sweeps(N, s[r], int(seeds[r]), tab, N_SWEEPS, FIRST) for r in range(n)]
        want = {k: np.stack([np.asarray(r[k]) for r in rows]) for k in hu.FIELDS + ("energy_hist",)}
        got = tu.host_with_table(N, s, seeds, tab, FIRST, True)
        hu.assert_equal(got, want, what, hist=True)
        zero = [sum(1 for w in r["words"] if w[2] == 0) for r in rows]
        live = [sum(1 for w in r["words"] if w[2] > 0) for r in rows]
        if name in tu.ZERO_ROWS:
            assert live == [0] * n, what
            assert (want["state"] == N - 1).all() and (got["state"] == N - 1).all(), f"{what}: W = 0 sends every column to the height N - 1"
        elif name == "only1":
            both = any(z > 0 and v > 0 for z, v in zip(zero, live))
            assert both == (N in BOTH_BOARD), f"{what}: W = 0 updates {zero}, W > 0 updates {live}"
        elif name == "altzero":
            assert zero == [N * N] * n, what
            np.testing.assert_array_equal(want["energy_hist"][:, 2], np.full(n, qu.energy(N, np.full(N * N, N - 1))), err_msg=what)  # all heights N - 1 after the zero row
        elif name != "only3":
            assert zero == [0] * n and (want["n_changed"] > 0).all(), what
        if name == "ones":
            assert all(w[2] == N for r in rows for w in r["words"]), what
        if name == "full":
            assert all(w[2] == N * B for r in rows for w in r["words"]), what


def test_an_entry_above_two_to_the_24_is_refused_by_the_host_entry_points():
    L = mcq_amd._lib.lib()
    n, n_sweeps, D = 2, 3, 4
    sd = np.arange(n, dtype=np.uint32)
    boards = np.zeros((n, 36), dtype=np.uint8)
    cubes = q3.random_placements(6, n, 1)
    out_b, out_c = np.zeros_like(boards), np.zeros_like(cubes)

    def board(tab):
        q = abi.Heatbath()
        q.N, q.mode, q.n_chains, q.n_sweeps, q.first_sweep, q.table_len = 6, abi.MODE_BOARD, n, n_sweeps, 0, D
        q.seeds, q.table, q.state_in, q.state_out = sd.ctypes.data, tab.ctypes.data, boards.ctypes.data, out_b.ctypes.data
        return q

    def cube(tab):
        q = abi.Heatbath3D()
        q.N, q.n_queens, q.n_chains, q.n_sweeps, q.first_sweep, q.table_len = 6, 0, n, n_sweeps, 0, D
        q.seeds, q.table, q.state_in, q.state_out = sd.ctypes.data, tab.ctypes.data, cubes.ctypes.data, out_c.ctypes.data
        return q

    for block, fn, err in ((board, L.mcq_heatbath_host, L.mcq_heatbath_last_error), (cube, L.mcq_heatbath3d_host, L.mcq_heatbath3d_last_error)):
        ok = np.full((n_sweeps, D), B, dtype=np.uint32)  # exactly 2^24 everywhere: accepted
        assert fn(ctypes.byref(block(ok))) == abi.OK, err()
        for value in (B + 1, 2**32 - 1):
            for s, d in ((0, 0), (0, D - 1), (n_sweeps - 1, 0), (n_sweeps - 1, D - 1), (1, 2)):
                tab = np.full((n_sweeps, D), 5, dtype=np.uint32)
                tab[s, d] = value
                assert fn(ctypes.byref(block(tab))) == abi.EINVAL, (value, s, d)
                msg = err().decode()
                assert "table" in msg and f"sweep {s} " in msg and f"index {d} " in msg and str(value) in msg and "2^24" in msg, msg
                tab[s, d] = B
                assert fn(ctypes.byref(block(tab))) == abi.OK
    # rows beyond n_sweeps are not the call's: they are not read
    tab = np.full((n_sweeps + 1, D), 5, dtype=np.uint32)
    tab[n_sweeps] = 2**32 - 1
    assert L.mcq_heatbath_host(ctypes.byref(board(tab))) == abi.OK and L.mcq_heatbath3d_host(ctypes.byref(cube(tab))) == abi.OK
    # the Python wrappers raise it
    with pytest.raises(ValueError, match="table"):
        tu.host_with_table(6, boards, sd, np.full((1, 2), B + 1, dtype=np.uint32), 0, False)
    with pytest.raises(ValueError, match="table"):
        tu.host3d(6, 36, cubes, sd, np.full((1, 2), B + 1, dtype=np.uint32), 1)
    assert int(abi.heatbath_table([0.0, 0.3, 50.0]).max()) == B  # what the Python side builds stays inside the bound
