"""GPU: the three tempering kernels -- mcq_temper_kernel (form "lines"), mcq_temper_counters_kernel (form "counters") and the kernel of
csrc/mcq_temper3d.hip -- against the library's host code bit for bit on every output and both histories, on weight and swap tables of
the CALLER's (tests/temper_tables_util.py) that abi.temper_tables never builds.  At one (N, R) per instantiation and per path of the
launch: rows that differ from rung to rung (`mixed`: W = 0 rows, T[0] = 0, a clip onto a live entry, non-monotone rows, a zero row
between live ones, another row per sweep) under swap rows drawn over the full 32 bits and under [0, 0, M]; one family on every rung
under the rising ramp; the pair's own word as the swap row (nothing swaps below Delta = 0) and that word plus one (every pair swaps),
with every ladder's slot 0 seeded alike; D = 512 of 2^24 on one rung where the LDS is fullest; and the exchange stream's word index
across 2^34, whole and cut at the crossing with the rungs carried on the device.

The kernels share pair_swaps and exchange_word with the host code: tests/test_temper_tables_host.py holds those to the restatements on
the same tables.  What a comparison must contain is asserted from the host code's outputs."""
import functools

import numpy as np
import pytest

import mcq_amd
from tests import temper3d_util as t3
from tests import temper_tables_util as tt
from tests import temper_util as tu

abi = mcq_amd.abi
tempering = mcq_amd.tempering
pytestmark = pytest.mark.gpu

# (N, R, Q).  lines: both sides of the six instantiations' borders and (2, 2) with 3 ladders, two ladders per workgroup and half of one
# empty; counters: every (padded N, R) instantiation; full_3d: one pair per instantiation of tests/test_temper3d.py and the near-full cube
LINES = ((2, 2), (8, 16), (12, 4), (13, 2), (16, 16), (17, 8), (24, 2), (32, 16), (33, 4), (64, 2))
COUNTERS = ((3, 2), (8, 16), (12, 4), (16, 16), (6, 4), (5, 8), (9, 2), (10, 8), (11, 16), (13, 2), (14, 4), (15, 8))
CUBES = ((4, 16, 16), (12, 2, 144), (13, 4, 169), (13, 8, 169), (16, 16, 256), (20, 2, 400), (20, 4, 400), (20, 8, 400), (3, 4, 26))
PAIRS = {"lines": tuple((N, R, None) for N, R in LINES), "counters": tuple((N, R, None) for N, R in COUNTERS), "cube": CUBES}
# D = 512 on one rung: where the LDS of a ladder is fullest
FULL = {"lines": ((12, 16, None), (33, 4, None)), "counters": ((16, 16, None),), "cube": ((12, 16, 144), (20, 8, 400))}
WORD = {"lines": (12, None), "counters": (12, None), "cube": (4, 16)}  # the word-index case: R = 16
RUNS = ("mixed x rand", "mixed x clip", "same x ramp", "aimed + 0", "aimed + 1")


def _kind(kernel):
    return "cube" if kernel == "cube" else "board"


def _host(kernel, N, Q, s, seeds, T, X, K, first, rungs):
    return tu.host_call(N, s, seeds, T, X, K, first, rungs) if Q is None else t3.host_call(N, Q, s, seeds, T, X, K, first, rungs)


def _device(kernel, N, Q, s, seeds, T, X, K, first, rungs, tensors=False):
    if tensors:  # the tables and the rungs handed over as device tensors
        import torch

        dev = torch.device("cuda", torch.cuda.current_device())
        T, X = tt.device_tables(T, X, dev)
        rungs = None if rungs is None else torch.from_numpy(rungs).to(dev)
    return tt.own_tables(N, s, seeds, T, X, K, first, rungs, form=kernel if Q is None else None, Q=Q)


def _same(got, want, what):
    (tu if "flags" not in want else t3).assert_equal(got, want, what, hist=True)
    assert set(got) == set(want), what
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)


def _shape(kernel, idx):
    """(ladders, sweeps, K, first_sweep, rung_in given) of the idx-th pair: 1 to 3 ladders (3 at R = 2, where two ladders share a workgroup
    of the board kernels and an event looks at one pair or at none), 3 to 6 sweeps (3, and one ladder beyond R = 2, where the host code
    is the slow side), K = 1 or 2 (1 at R = 2), first_sweep off a multiple of K."""
    N, R, Q = PAIRS[kernel][idx]
    slow = N >= 33 or (Q is not None and N >= 20)
    ladders = 3 if R == 2 or idx == 0 else 1 if slow else 1 + idx % 3
    K = 1 if R == 2 else 1 + idx % 2
    return ladders, (3 if slow else 6 if idx == 0 else 3 + idx % 4), K, 2 * (idx % 3) + 1, idx % 2 == 1


@functools.lru_cache(maxsize=None)
def _case(kernel, idx):
    """{run: (arguments, the host code's result)} of the idx-th pair of the kernel: computed once, shared, left unchanged."""
    N, R, Q = PAIRS[kernel][idx]
    ladders, n_sweeps, K, first, given = _shape(kernel, idx)
    n, kind = R * ladders, _kind(kernel)
    s, seeds = tt.placements(kind, N, Q, n, 47 * N + R), abi.seeds_for(4200000000 + 100 * N + R, n)
    rungs = tt.rungs(n, R, N + R) if given else None
    n_events = tu.events(first, n_sweeps, K)
    W, X = tt.ladder_tables(n_sweeps, R), tt.swap_tables(n_events, R, N + R)
    family = tt.FAMILIES[idx % len(tt.FAMILIES)]
    alike = seeds.copy()
    alike[::R] = seeds[0]  # every ladder's slot 0 seeded alike: one aimed table serves them all
    runs = {"mixed x rand": (s, seeds, W["mixed"], X["rand"], K, first, rungs), "mixed x clip": (s, seeds, W["mixed"], X["clip"], K, first, rungs),
            "same x ramp": (s, seeds, W["same:" + family], X["ramp"], K, first, rungs)}
    for bump in (0, 1):
        runs[f"aimed + {bump}"] = (s, alike, W["mixed"], tt.aimed(alike[0], R, first // K, n_events, 3 if Q is None else 4, bump), K, first, rungs)
    assert tuple(runs) == RUNS
    return {name: (a, _host(kernel, N, Q, *a)) for name, a in runs.items()}


def test_the_pairs_cover_every_instantiation_and_every_family():
    """From the launch code of csrc/mcq_temper.hip and csrc/mcq_temper3d.hip, without a GPU."""
    lines = lambda N: (16, 8) if N <= 8 else (16, 12) if N <= 12 else (16, 16) if N <= 16 else (32, 24) if N <= 24 else (32, 32) if N <= 32 else (64, 64)  # noqa: E731
    assert {lines(N) for N, R in LINES} == {(16, 8), (16, 12), (16, 16), (32, 24), (32, 32), (64, 64)}
    assert all({lines(N), lines(N + 1)} <= {lines(n) for n, _ in LINES} for N in (8, 12, 16, 24, 32))  # both sides of every border but 8 | 9
    assert any(R * lines(N)[0] < 64 for N, R in LINES) and LINES[0] == (2, 2) and _shape("lines", 0)[0] == 3  # two ladders per workgroup
    assert {R for _, R in LINES} == set(abi.TEMPER_REPLICAS)
    pad = lambda N: 8 if N <= 8 else 12 if N <= 12 else 16  # noqa: E731
    assert {(pad(N), R) for N, R in COUNTERS} == {(p, R) for p in (8, 12, 16) for R in abi.TEMPER_REPLICAS} and max(N for N, _ in COUNTERS) == abi.MAX_N_TEMPER_COUNTERS
    assert COUNTERS[0] == (3, 2) and all(_shape(k, i)[0] == 3 for k, p in PAIRS.items() for i in range(len(p)) if p[i][1] == 2)
    lanes = lambda N, R: min(64 if N <= 12 else 256 if N <= 19 else 1024, 1024 // R)  # noqa: E731  (tests/test_temper3d.py: test_every_instantiation_is_reached)
    inst = [(lanes(N, R), 8 if N <= 19 else 16, 32 if N <= 12 else 64) for N, R, Q in CUBES if Q == N * N]
    assert sorted(inst) == sorted([(64, 8, 32), (64, 8, 32), (256, 8, 64), (128, 8, 64), (64, 8, 64), (512, 16, 64), (256, 16, 64), (128, 16, 64)])
    assert all(t3.fits(N, R, Q, 512) for N, R, Q in CUBES) and CUBES[-1] == (3, 4, 26) and 3 ** 3 - 26 == 1
    for kernel, pairs in PAIRS.items():
        assert {tt.FAMILIES[i % 8] for i in range(len(pairs))} == set(tt.FAMILIES), kernel
        shapes = [_shape(kernel, i) for i in range(len(pairs))]
        assert all(1 <= c[0] <= 3 and 3 <= c[1] <= 6 and (c[2] == 1 or c[3] % c[2]) for c in shapes) and {c[4] for c in shapes} == {True, False}
    # D = 512 on one rung: the largest R that fits beside it at N = 12 and N = 20
    assert [max(R for R in abi.TEMPER_REPLICAS if t3.fits(N, R, N * N, 512)) for N in (12, 20)] == [16, 8] == [R for _, R, _ in FULL["cube"]]
    assert abi.temper_counters_lds_bytes(16, 16, 512) == 154816


IDS = [(kernel, idx) for kernel, pairs in PAIRS.items() for idx in range(len(pairs))]


@pytest.mark.parametrize("kernel,idx", IDS, ids=[f"{k}-N{PAIRS[k][i][0]}-R{PAIRS[k][i][1]}" + (f"-Q{PAIRS[k][i][2]}" if k == "cube" else "") for k, i in IDS])
def test_kernel_equals_the_host_code_on_a_callers_tables(kernel, idx):
    N, R, Q = PAIRS[kernel][idx]
    case = _case(kernel, idx)
    ladders, n_sweeps, K, first, given = _shape(kernel, idx)
    what = f"{kernel} N={N} R={R} Q={Q}, {ladders} ladders, K={K}, {n_sweeps} sweeps from {first}, rung_in={'given' if given else 'default'}"
    # from the host code alone: the sweeps moved, the rungs moved, the run that never swaps below Delta = 0 and the one that always does
    # differ (a pair with Delta < 0 was looked at), and where every rung holds one family the histories do not depend on the rungs
    for name in RUNS:
        want = case[name][1]
        assert "flags" not in want or not want["flags"].any(), (what, name)
        # (W = 0 on every update leaves a queen of full_3d where it is: rule item 3 of mcq_heatbath3d)
        assert want["n_changed"].sum() > 0 or (Q is not None and name == "same x ramp" and tt.FAMILIES[idx % len(tt.FAMILIES)] == "zero3"), (what, name)
    assert sum(int(case[name][1]["n_exchanges"].sum()) for name in RUNS[:3]) > 0, what
    if N == 2 and Q is None:  # every 2 x 2 board has the energy 6: Delta = 0 at every pair, and the two aimed runs are one
        assert all((case[name][1]["energy_hist"] == 6).all() for name in RUNS)
    else:
        assert (case["aimed + 0"][1]["rung_hist"] != case["aimed + 1"][1]["rung_hist"]).any(), what
    tt.assert_swaps_follow(case["aimed + 0"][1], R, K, first, lambda d: d >= 0)
    np.testing.assert_array_equal(case["aimed + 1"][1]["rung_hist"], tt.transposition_rungs(R, case["aimed + 1"][1]["rung_hist"][:, 0], first, n_sweeps, K))
    for j, name in enumerate(RUNS):
        args, want = case[name]
        _same(_device(kernel, N, Q, *args, tensors=j % 2 == idx % 2), want, f"{what}: {name}")


FULL_IDS = [(kernel, i) for kernel, pairs in FULL.items() for i in range(len(pairs))]


@pytest.mark.parametrize("kernel,i", FULL_IDS, ids=[f"{k}-N{FULL[k][i][0]}-R{FULL[k][i][1]}" for k, i in FULL_IDS])
def test_a_full_row_on_one_rung(kernel, i):
    """mixed_full: rung 0 holds 512 entries of 2^24 -- the largest W and the largest partial sums the bound allows -- and the other rungs
    the rows of `mixed`, padded to 512: the most LDS a ladder of this shape takes, and the slot on rung 0 changes as the pairs swap."""
    N, R, Q = FULL[kernel][i]
    ladders, n_sweeps, K, first = 2 if N < 20 else 1, 3 if N >= 20 else 4, 1, 2
    n = R * ladders
    s, seeds, rungs = tt.placements(_kind(kernel), N, Q, n, 7 * N + R), abi.seeds_for(4250000000 + N, n), tt.rungs(n, R, N)
    T = tt.ladder_tables(n_sweeps, R)["mixed_full"]
    for j, x in enumerate(("rand", "max1")):
        X = tt.swap_tables(n_sweeps, R, N)[x]
        want = _host(kernel, N, Q, s, seeds, T, X, K, first, rungs)
        assert want["n_changed"].sum() > 0 and want["n_exchanges"].sum() > 0
        assert x != "max1" or len({int(r) for r in np.nonzero(want["rung_hist"] == 0)[0]}) > ladders  # rung 0 went from slot to slot
        _same(_device(kernel, N, Q, s, seeds, T, X, K, first, rungs, tensors=j == 1), want, f"{kernel} N={N} R={R}, mixed_full x {x}")


@pytest.mark.parametrize("kernel", tuple(WORD))
def test_the_word_index_crosses_2_to_the_34_on_the_device(kernel):
    """R = 16, K = 1, first_sweep = 2^30 - 3, 6 sweeps: the kernel's exchange words on either side of e R + t = 2^34, in one launch and
    in two cut at the crossing, the placements and the rungs carried on the device."""
    import torch

    N, Q = WORD[kernel]
    R, first, n_sweeps, cut = tt.WORD_R, tt.WORD_FIRST, tt.WORD_SWEEPS, 3
    s, seeds, T, X, rungs = tt.word_case(_kind(kernel), N, Q, 2)
    want = _host(kernel, N, Q, s, seeds, T, X, 1, first, rungs)
    sides = tt.word_sides(want)
    print(f"{kernel}: {sides[0]} words drawn below 2^34 and {sides[1]} from it on")
    assert min(sides) >= 3 and want["n_exchanges"].sum() > 0
    whole = _device(kernel, N, Q, s, seeds, T, X, 1, first, rungs)
    _same(whole, want, f"{kernel} N={N} across 2^34")
    dev = torch.device("cuda", torch.cuda.current_device())
    t, rung = torch.from_numpy(s).to(dev), torch.from_numpy(rungs).to(dev)
    parts = []
    for a, b in ((0, cut), (cut, n_sweeps)):
        tabs = tt.device_tables(T[a:b], X[a:b], dev)
        kw = dict(tables=tabs, exchange_every=1, first_sweep=first + a, rungs=rung, out=t, trace=True)
        res = tempering.temper_device(N, t, seeds, form=kernel, **kw) if Q is None else tempering.temper_queens_device(N, t, seeds, Q=Q, **kw)
        torch.cuda.current_stream(dev).synchronize()
        assert res["state"] is t
        rung = res["rung_out"]
        parts.append(tempering.to_numpy(res))
    tt.assert_cut_equals_whole(parts[0], parts[1], want, cut, f"{kernel} N={N} cut at the crossing")
