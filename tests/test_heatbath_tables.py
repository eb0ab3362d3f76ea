"""GPU: the three heat-bath kernels (mcq_heatbath3d_device, mcq_heatbath_device, mcq_heatbath_counters_device) on weight tables that a
CALLER builds -- the families of tests/heatbath_tables_util.py, which abi.heatbath_table never produces: W = 0 on some updates and not on
others, a non-zero entry behind the clip, one entry, rows that change and vanish from sweep to sweep, 512 entries of 2^24 -- against
the library's host codes bit for bit on every output (tests/test_heatbath_tables_host.py holds those against the restatements on the
same tables), and the full_3d heat-bath and quench kernels on near-full cubes up to N = 32 with N^3 - 1 queens, the largest dynamic
LDS request either of them makes."""
import numpy as np
import pytest

import mcq_amd
from tests import heatbath3d_util as h3
from tests import heatbath_tables_util as tu
from tests import heatbath_util as hu
from tests import quench3d_util as q3
from tests.test_heatbath import _boards, _seeds
from tests.test_heatbath3d import _placements

abi = mcq_amd.abi
heatbath = mcq_amd.heatbath
quench = mcq_amd.quench
pytestmark = pytest.mark.gpu
B = tu.B
FIRSTS_3D = (0, 5, (1 << 33) + 3)


def _device():
    import torch

    return torch.device("cuda", torch.cuda.current_device())


def _queens_on_device(N, Q, s, seeds, tab, first):
    """heatbath_queens_device with the caller's table uint32[n_sweeps][D] uploaded as it is, every output as NumPy."""
    import torch

    dev = _device()
    dtab = torch.from_numpy(tab.view(np.int32)).to(dev)
    res = heatbath.heatbath_queens_device(N, torch.from_numpy(np.ascontiguousarray(s)).to(dev), seeds, dtab, Q=Q, first_sweep=first, trace=True)
    torch.cuda.current_stream(dev).synchronize()
    return heatbath.to_numpy(res)


# both ends of each instantiation of the full_3d kernel: (N, Q, chain counts, sweeps).  (32, 2) with `full` is the largest sum a lane
# holds (34 entries of 2^24) and W ~ 2^39; (12, 2) and (13, 2) with `ones` are the smallest non-zero W, on whole wavefronts of lanes
# that own no weight
SHAPES_3D = [(N, Q, (1, 5), 3) for N, Q in ((2, 4), (3, 9), (5, 25), (8, 64), (12, 144), (12, 2), (12, 1727))] + \
            [(N, Q, (3,), 2) for N, Q in ((13, 169), (13, 2), (19, 361))] + [(N, Q, (1, 3), 1) for N, Q in ((20, 400), (32, 200), (32, 2))]


@pytest.mark.parametrize("N,Q,counts,n_sweeps", SHAPES_3D, ids=[f"{N}-{Q}" for N, Q, _, _ in SHAPES_3D])
def test_full_3d_kernel_equals_the_host_code_on_every_family(N, Q, counts, n_sweeps):
    tabs = tu.tables(n_sweeps)
    for idx, n in enumerate(counts):
        s = _placements(N, n, 300 * N + Q % 7 + idx, Q=Q).reshape(n, Q, 3)  # n > 2: chain 1 holds a repeated cell; n > 4: chain 3 is all 255
        seeds = abi.seeds_for(17 * N + idx, n)
        for t, (name, tab) in enumerate(tabs.items()):
            st = s.copy()
            if n == 3 and t % 2:
                st[1] = 255  # three chains: the repeated chain is the all-255 one for every other family
            flags = [int(n > 2 and r == 1 or n > 4 and r == 3) for r in range(n)]
            first = FIRSTS_3D[(t + idx) % 3]
            what = f"N={N} Q={Q}, {n} chains, table {name}, first_sweep={first}"
            want = tu.host3d(N, Q, st, seeds, tab, n_sweeps, first)
            got = _queens_on_device(N, Q, st, seeds, tab, first)
            h3.assert_equal(got, want, what, hist=True)
            assert list(got["flags"]) == flags, what
            if name in tu.ZERO_ROWS:
                assert not got["n_changed"].any(), what
                np.testing.assert_array_equal(got["state"].reshape(n, -1), np.minimum(st, N - 1).reshape(n, -1), err_msg=what)
            if N <= 8 and n == 1 and name in ("only1", "altzero"):  # against the restatement too, where it is quick
                h3.assert_equal(got, h3.sweeps_many(N, st, seeds, None, Q=Q, first_sweep=first, tab=tab), what + " vs the restatement", hist=True)


def test_full_3d_one_entry_makes_every_update_uniform_on_the_device():
    """Rule item 7, D = 1: the new cell is the floor(x F / 2^64)-th candidate in index order, whatever the entry; in Python integers."""
    for idx, (N, Q) in enumerate(((5, 100), (13, 30), (20, 10))):
        n, n_sweeps, first = 2, 2, (0, 11, 5)[idx]
        s = q3.random_placements(N, n, 650 + idx, Q=Q)
        seeds = abi.seeds_for(9 + idx, n)
        F = N ** 3 - Q + 1
        want = []
        for r in range(n):
            z = q3.clamp(N, s[r]).copy()
            for sw in range(n_sweeps):
                for q in range(Q):
                    free = np.setdiff1d(np.arange(N ** 3), np.delete(h3.cell_index(N, z), q))
                    assert len(free) == F
                    z[q] = q3._cells(N)[int(free[(h3.draw(int(seeds[r]), (first + sw) * Q + q) * F) >> 64])]
            want.append(z.astype(np.uint8).reshape(-1))
        for t0 in (1, B):
            got = _queens_on_device(N, Q, s, seeds, np.full((n_sweeps, 1), t0, dtype=np.uint32), first)
            np.testing.assert_array_equal(got["state"], np.stack(want), err_msg=f"N={N} Q={Q} T=[{t0}]")
            assert [int(e) for e in got["energy_out"]] == [q3.energy(N, w) for w in want] and not got["flags"].any()


def test_full_3d_segments_under_a_callers_table():
    """Two device calls on the rows [:1] and [1:] of one table, first_sweep carried over, the second in place, against ONE host call."""
    import torch

    dev = _device()
    for idx, (N, Q) in enumerate(((6, 36), (16, 256))):
        n, n_sweeps, first = 4, 3, 7 + idx
        tab = tu.tables(n_sweeps)["rand"]
        s = _placements(N, n, 80 + idx, Q=Q)
        seeds = abi.seeds_for(21 + idx, n)
        whole = tu.host3d(N, Q, s, seeds, tab, n_sweeps, first)
        dtab = torch.from_numpy(tab.view(np.int32)).to(dev)
        t = torch.from_numpy(s).to(dev)
        a = heatbath.heatbath_queens_device(N, t, seeds, dtab[:1], Q=Q, first_sweep=first, trace=True)
        b = heatbath.heatbath_queens_device(N, a["state"], seeds, dtab[1:], Q=Q, first_sweep=first + 1, out=a["state"], trace=True)
        torch.cuda.current_stream(dev).synchronize()
        assert b["state"].data_ptr() == a["state"].data_ptr()
        ga, gb = heatbath.to_numpy(a), heatbath.to_numpy(b)
        what = f"N={N} Q={Q}: segments of a caller's table"
        np.testing.assert_array_equal(gb["state"], whole["state"], err_msg=what)
        np.testing.assert_array_equal(np.concatenate([ga["energy_hist"], gb["energy_hist"][:, 1:]], axis=1), whole["energy_hist"], err_msg=what)
        np.testing.assert_array_equal(gb["energy_out"], whole["energy_out"], err_msg=what)
        np.testing.assert_array_equal(ga["n_changed"] + gb["n_changed"], whole["n_changed"], err_msg=what)
        np.testing.assert_array_equal(np.minimum(ga["best_energy"], gb["best_energy"]), whole["best_energy"], err_msg=what)
        np.testing.assert_array_equal(gb["flags"], whole["flags"], err_msg=what)
        assert whole["n_changed"][0] > 0 and list(whole["flags"]) == [0, 1, 0, 0]


def _near_full(N, Q, n):
    """n placements of Q queens on distinct cells; with two chains the second holds one repeated cell."""
    s = q3.random_placements(N, n, N + Q, Q=Q).reshape(n, Q, 3)
    if n > 1:
        s[1, Q - 1] = s[1, 0]
    return s.reshape(n, 3 * Q)


@pytest.mark.parametrize("N,Q,n", ((19, 6858, 1), (19, 6000, 1), (32, 32767, 2)))
def test_near_full_cubes_heat_bath(N, Q, n):
    """One sweep of a cube with few free cells: the field's counts are at their largest (13 * 18 + 1 = 235 in a byte at N = 19) and
    a - a_min reaches far into the table.  (32, 32 767) is the kernel's largest dynamic LDS request, 137 504 bytes; its second chain
    holds a repeated cell: flagged, recounted, handed back unmoved."""
    s, seeds = _near_full(N, Q, n), abi.seeds_for(N, n)
    flags = [0, 1][:n]
    want = heatbath.heatbath_queens_host(N, s, seeds, [0.7], Q=Q, first_sweep=3, trace=True)
    got = heatbath.heatbath_queens(N, s, seeds, [0.7], Q=Q, first_sweep=3, trace=True)
    h3.assert_equal(got, want, f"N={N} Q={Q}, beta = 0.7", hist=True)
    assert list(got["flags"]) == flags and int(abi.heatbath_table([0.7]).shape[1]) > 20
    full = tu.tables(1)["full"]
    wantf = tu.host3d(N, Q, s, seeds, full, 1, 3)
    gotf = _queens_on_device(N, Q, s, seeds, full, 3)
    h3.assert_equal(gotf, wantf, f"N={N} Q={Q}, 512 entries of 2^24", hist=True)
    assert list(gotf["flags"]) == flags and int(gotf["n_changed"][0]) > 0
    if n > 1:
        for g in (got, gotf):
            assert int(g["n_changed"][1]) == 0 and int(g["energy_in"][1]) == int(g["energy_out"][1]) == int(want["energy_in"][1])
            np.testing.assert_array_equal(g["state"][1], s[1])


def test_near_full_cube_quench_at_the_largest_lds_request():
    """The full_3d quench at N = 32 with 32 767 queens (132 KiB of dynamic LDS): one pass and until nothing moves, and a repeated chain."""
    N, Q, n = 32, 32767, 2
    s = _near_full(N, Q, n)
    for max_passes in (1, 0):
        want = quench.quench_queens_host(N, s, Q=Q, max_passes=max_passes)
        got = quench.quench_queens(N, s, Q=Q, max_passes=max_passes)
        q3.assert_equal(got, want, f"N={N} Q={Q} max_passes={max_passes}")
        assert list(got["flags"]) == [0, abi.QUENCH3D_REPEATED] and int(got["n_moves"][1]) == 0
        np.testing.assert_array_equal(got["state"][1], s[1])
        assert int(got["energy_in"][1]) == int(got["energy_out"][1]) == int(want["energy_in"][1])
    assert int(got["n_moves"][0]) > 0


def _boards_on_device(N, s, seeds, tab, first, form):
    import torch

    dev = _device()
    dtab = torch.from_numpy(tab.view(np.int32)).to(dev)
    res = heatbath.heatbath_device(N, torch.from_numpy(np.ascontiguousarray(s)).to(dev), seeds, dtab, first_sweep=first, trace=True, form=form)
    torch.cuda.current_stream(dev).synchronize()
    return heatbath.to_numpy(res)


def _board_families(N, counts, n_sweeps, forms):
    tabs = tu.tables(n_sweeps)
    for idx, n in enumerate(counts):
        s, seeds = _boards(N, n, 100 * N + idx), _seeds(n, N + idx)  # chain 0 all-equal heights, chain 1 (n > 2) all 255
        for t, (name, tab) in enumerate(tabs.items()):
            first = (0, 3, (1 << 34) // (N * N) + 5, 1 << 40)[(idx + t) % 4]
            what = f"N={N}, {n} chains, table {name}, first_sweep={first}"
            want = tu.host_with_table(N, s, seeds, tab, first, True)
            gots = [_boards_on_device(N, s, seeds, tab, first, form) for form in forms]
            for form, got in zip(forms, gots):
                hu.assert_equal(got, want, f"{what}: {form} vs the host code", hist=True)
                hu.assert_equal(got, gots[-1], f"{what}: {form} vs {forms[-1]}", hist=True)
                if name in tu.ZERO_ROWS:
                    assert (got["state"] == N - 1).all(), f"{what}: W = 0 sends every column to the height N - 1"


# one N per instantiation of the lines form and the ends that differ; N = 65 and 128 hold two heights per lane, kn from two ballots
@pytest.mark.parametrize("N", (2, 8, 12, 16, 17, 24, 32, 33, 64, 65, 128))
def test_board_lines_kernel_equals_the_host_code_on_every_family(N):
    _board_families(N, (1, 5, 17) if N <= 33 else (1, 3), 3 if N <= 33 else 2, ("lines",))


@pytest.mark.parametrize("N", (2, 8, 9, 12, 13, 16))
def test_board_counters_kernel_equals_the_lines_kernel_and_the_host_code_on_every_family(N):
    _board_families(N, (1, 5, 17), 3, ("counters", "lines"))
