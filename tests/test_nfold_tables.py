"""GPU: the n-fold kernels (mcq_nfold_device, mcq_nfold3d_device) against the library's host code bit for bit on every output and
dtype, on weight rows and clocks of the CALLER's (tests/nfold_tables_util.py) that nfold.weight_tables and nfold.clock_tables never
build: every family under both clocks, three segments and nine chains at both ends of the six board instantiations and at eight cubes
over the three workgroup sizes and both field packings; the closed form under the row [1] and the clock of ones over thousands of
one-event chains whose draws reach the first and the last column of every lane's chunk (boards) and the first and the last busy lane's
run of cells and of queens (full_3d); and rows and clock handed over as device tensors.  tests/test_nfold_tables_host.py holds the host
code to the NumPy restatements on the same families.

What each family is there to reach (the kernels' lines are named in tests/nfold_tables_util.py: rows):
  the draw at a prefix boundary -- `incl > U`, `u < r`, `pk > u32` of csrc/mcq_nfold.hip; `before <= U && U - before < own` and its cell
      twin, `u < r`, `pre > u` and the hand-over of u through win[1..2] of csrc/mcq_nfold3d.hip: ones (every U is the first and the last
      integer of its move), small, up_only, rising, and the closed form
  R(q) = G(c_q) + corr(q), `r += T[dd - 1] - T[dd]` in step (3) of csrc/mcq_nfold3d.hip: rising (every term negative), small, nonmono
  the high clamp on a non-zero entry, T[0] != 2^24, R = 0 between live columns or queens, D = 1: clip, rising, nonmono, up_only, only3, ones
  small W and small need, tau = max(1, ...) with W > 0: every family under the clocks "unit" and "exp16" (entries of 0)
  rows that change character between segments: altzero (live, zero, live), rand (another row per segment)

The host code's events are cut where they would take seconds: under the families of tu.HEAVY a segment is one step, and at the larger
shapes their chains carry a need, aimed from the host code's own weight_out, with which they sleep through two segments and fire
within the last 150 (boards) or 60 (full_3d) units of the third."""
import functools

import numpy as np
import pytest

import mcq_amd
from tests import nfold3d_util as n3
from tests import nfold_tables_util as tu
from tests import quench3d_util as q3
from tests import quench_util as qu

abi = mcq_amd.abi
nfold = mcq_amd.nfold
pytestmark = pytest.mark.gpu

SIZES = (2, 4, 5, 8, 9, 12, 13, 16, 17, 24, 25, 32)  # both ends of the six instantiations, padded N = 4, 8, 12, 16, 24, 32
CUBES = ((3, 4), (6, 36), (12, 37), (12, 144), (13, 11), (19, 23), (20, 7), (32, 5))  # 64, 256 and 1024 lanes; 4 and 2 cells per dword
CHAINS, SEGS, LIGHT_STEPS, TICKS, CUBE_TICKS = 9, 3, 6, 150, 60
SPARSE = tuple(c for c in CUBES if c[1] <= 2 * c[0])  # so few queens that no free cell sees three more of them than a queen does
CLOCKS = tuple(tu.clocks())


def _assert_same(got, want, what, fields):
    for k in fields:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].dtype, want[k].dtype)
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{what}: {k}")


def _aim(host, rows, n, sleeping_need, ticks):
    """need_in uint64[n]: the chains sleep through all segments of one step but the last and fire `ticks` units before its end.  W of the
    input under every row is the host code's weight_out of a run of that row alone that a large need keeps asleep."""
    sleep = np.full(n, sleeping_need, dtype=np.uint64)
    w = np.stack([host(rows[i : i + 1], sleep) for i in range(len(rows))], axis=1)
    return np.array([tu.aimed_need(w[r], ticks) for r in range(n)], dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def _board_case(N, clock):
    """{family: (placements with bytes >= N, seeds, rows, steps, need_in, the host code's result)}: computed once, shared, left unchanged."""
    s = qu.random_boards(N, CHAINS, 600 + N, over=True)
    seeds = abi.seeds_for(4100000000 + 100 * N, CHAINS)
    ck = tu.clocks()[clock]
    case = {}
    for family, rows in tu.rows(SEGS, abi.MAX_NFOLD_TABLE).items():
        steps, need = (1 if family in tu.HEAVY else LIGHT_STEPS), None
        if family in tu.HEAVY and N >= 12:
            rows = np.ascontiguousarray(np.roll(rows, -(N % SEGS), axis=0)) if family == "rand" else rows
            need = _aim(lambda row, sleep: nfold.nfold_states_host(N, s, seeds, row, 1, clock=ck, need_in=sleep)["weight_out"], rows, CHAINS, 1 << 44, TICKS)
        case[family] = (s, seeds, rows, steps, need, nfold.nfold_states_host(N, s, seeds, rows, steps, clock=ck, need_in=need, hist=True))
    return case


@pytest.mark.parametrize("clock", CLOCKS)
@pytest.mark.parametrize("N", SIZES)
def test_board_kernel_equals_the_host_code(N, clock):
    case = _board_case(N, clock)
    events = {family: int((c[5]["events_out"]).sum()) for family, c in case.items()}
    print(f"N = {N}, {clock}: events {events}")
    for family, (s, seeds, rows, steps, need, want) in case.items():
        assert events[family] > 0 or (N == 2 and family in ("only3", "up_only")), (family, events)  # (N = 2 has no difference of 3, and few rises)
        if family in ("rising", "clip") and N > 2:
            assert int(want["n_uphill"].sum()) > 0
        got = nfold.nfold_states(N, s, seeds, rows, steps, clock=tu.clocks()[clock], need_in=need, hist=True)
        _assert_same(got, want, f"N = {N}, {family}, {clock}", nfold.FIELDS)


@functools.lru_cache(maxsize=None)
def _cube_case(N, Q, clock):
    s = q3.random_placements(N, CHAINS, 600 + N + Q, Q=Q, over=True)
    seeds = abi.seeds_for(4100000000 + 100 * N + Q, CHAINS)
    ck = tu.clocks()[clock]
    case = {}
    for family, rows in tu.rows(SEGS, abi.MAX_NFOLD3D_TABLE).items():
        steps, need = (1 if family in tu.HEAVY else 16 if (N, Q) in SPARSE else 4), None  # (a sparse cube has few moves of weight)
        if family in tu.HEAVY and N >= 6:
            rows = np.ascontiguousarray(np.roll(rows, -(N % SEGS), axis=0)) if family == "rand" else rows
            need = _aim(lambda row, sleep: nfold.nfold_queens_host(N, s, seeds, row, 1, Q=Q, clock=ck, need_in=sleep)["weight_out"], rows, CHAINS, 1 << 57, CUBE_TICKS)
        case[family] = (s, seeds, rows, steps, need, nfold.nfold_queens_host(N, s, seeds, rows, steps, Q=Q, clock=ck, need_in=need, hist=True))
    return case


@pytest.mark.parametrize("clock", CLOCKS)
@pytest.mark.parametrize("N,Q", CUBES)
def test_cube_kernel_equals_the_host_code(N, Q, clock):
    case = _cube_case(N, Q, clock)
    events = {family: int((c[5]["events_out"]).sum()) for family, c in case.items()}
    print(f"(N, Q) = ({N}, {Q}), {clock}: events {events}")
    for family, (s, seeds, rows, steps, need, want) in case.items():
        assert (want["flags"] == 0).all()
        quiet = ((N, Q) == CUBES[0] and family in ("only3", "up_only")) or ((N, Q) in SPARSE and family == "only3")
        assert events[family] > 0 or quiet, (family, events)
        if family in ("rising", "clip") and (N, Q) not in SPARSE:
            assert int(want["n_uphill"].sum()) > 0
        got = nfold.nfold_queens(N, s, seeds, rows, steps, Q=Q, clock=tu.clocks()[clock], need_in=need, hist=True)
        _assert_same(got, want, f"(N, Q) = ({N}, {Q}), {family}, {clock}", nfold.FIELDS_3D)


@pytest.mark.parametrize("N,n", ((32, 16384), (13, 2048)))
def test_board_closed_form_on_the_device(N, n):
    """One step under the row [1] and the unit clock is ONE event per chain, on the first and last integer of its move."""
    s = qu.random_boards(N, n, 700 + N, over=True)
    seeds = abi.seeds_for(3100000000 + N, n)
    M = N * N * (N - 1)
    want, cols = tu.boards_after(N, s, seeds, 1)
    # from the closed form alone: every column is moved by some chain, the first and the last of every lane's chunk among them
    assert set(int(c) for c in cols.reshape(-1)) == set(range(N * N))
    got = nfold.nfold_states(N, s, seeds, tu.rows(1, abi.MAX_NFOLD_TABLE)["ones"], 1, clock=tu.clocks()["unit"])
    np.testing.assert_array_equal(got["state"], want)
    assert (got["events_out"] == 1).all() and (got["need_out"] == M).all() and (got["weight_out"] == M).all()


@pytest.mark.parametrize("N,Q", ((12, 37), (19, 23), (32, 5)))
def test_cube_closed_form_on_the_device(N, Q):
    n = 4096
    s = q3.random_placements(N, n, 700 + N, Q=Q, over=True)
    seeds = abi.seeds_for(3100000000 + N, n)
    M = Q * (N ** 3 - Q)
    want, drawn = tu.queens_after(N, Q, s, seeds, 1)
    # from the closed form and the kernel's shares alone: the draws reach the first and the last busy lane's run of queens and of cells
    (qa, qb), (qc, qd), (ta, tb), (tc, td) = n3.shares(N, Q)
    q, t = drawn[:, 0, 0], drawn[:, 0, 1]
    hits = [int(((q >= qa) & (q < qb)).sum()), int(((q >= qc) & (q < qd)).sum()), int(((t >= ta) & (t < tb)).sum()), int(((t >= tc) & (t < td)).sum())]
    print(f"(N, Q) = ({N}, {Q}): draws in the first / last lane's queens and cells {hits}")
    assert min(hits) > 0, hits
    got = nfold.nfold_queens(N, s, seeds, tu.rows(1, abi.MAX_NFOLD3D_TABLE)["ones"], 1, Q=Q, clock=tu.clocks()["unit"])
    np.testing.assert_array_equal(got["state"], want)
    assert (got["flags"] == 0).all() and (got["events_out"] == 1).all() and (got["need_out"] == M).all() and (got["weight_out"] == M).all()


def test_rows_and_clock_as_device_tensors():
    import torch

    dev = torch.device("cuda", torch.cuda.current_device())
    ln2, ct = tu.clocks()["exp16"]
    dct = torch.from_numpy(ct.view(np.int32)).to(dev)
    N, n = 5, 9
    s, seeds = qu.random_boards(N, n, 800 + N, over=True), abi.seeds_for(55, n)
    rows = tu.rows(SEGS, abi.MAX_NFOLD_TABLE)["rand"]
    res = nfold.nfold_device(N, torch.from_numpy(s).to(dev), seeds, torch.from_numpy(rows.view(np.int32)).to(dev), 1, clock=(ln2, dct), hist=True)
    torch.cuda.current_stream(dev).synchronize()
    _assert_same(nfold.to_numpy(res), nfold.nfold_states(N, s, seeds, rows, 1, clock=(ln2, ct), hist=True), "boards, device tensors", nfold.FIELDS)
    N, Q = 6, 36
    s = q3.random_placements(N, n, 800 + N, Q=Q, over=True)
    rows = tu.rows(SEGS, abi.MAX_NFOLD3D_TABLE)["rand"]
    res = nfold.nfold_queens_device(N, torch.from_numpy(s).to(dev), seeds, torch.from_numpy(rows.view(np.int32)).to(dev), 1, Q=Q, clock=(ln2, dct), hist=True)
    torch.cuda.current_stream(dev).synchronize()
    want = nfold.nfold_queens(N, s, seeds, rows, 1, Q=Q, clock=(ln2, ct), hist=True)
    assert (want["events_out"] > 0).all()
    _assert_same(nfold.to_numpy(res), want, "full_3d, device tensors", nfold.FIELDS_3D)
