"""CPU-only: the two tempering host entry points (mcq_temper_host, mcq_temper3d_host) on weight and swap tables of the CALLER's
(tests/temper_tables_util.py) that abi.temper_tables never builds, bit for bit on every output and both histories:

  against the NumPy restatements (tests/temper_util.py, tests/temper3d_util.py) for every weight table with three swap tables and for
      rows that differ from rung to rung with every swap table;
  against the plain heat-bath host code where every rung holds the same row, and slot by slot where no event falls in the call;
  the swap decision against a predicate of Delta under swap rows of 0 and 2^32 - 1, and at its very edge: rows that hold the pair's own
      word x (nothing swaps: `x < X` fails by one) and x + 1 (everything swaps);
  the rungs against odd-even transposition under a table with which every pair swaps;
  the exchange stream's word index e R + t across 2^34, where the high counter word of its Philox block first leaves 0.

pair_swaps and exchange_word are shared by the kernels and the host code, so the kernel-against-host tests (tests/test_temper_tables.py)
cannot see them: these tests can."""
import numpy as np
import pytest

import mcq_amd
from tests import heatbath_tables_util as ht
from tests import quench_util as qu
from tests import temper3d_util as t3
from tests import temper_tables_util as tt
from tests import temper_util as tu

abi = mcq_amd.abi
heatbath = mcq_amd.heatbath
KINDS = ("board", "cube")
SHAPES = {"board": ((2, None), (3, None), (5, None)), "cube": ((2, 4), (3, 9), (4, 16), (2, 3), (3, 5), (4, 20))}  # (N, Q): Q = N^2 and one other
REPLICAS = (2, 4, 16)
HIST = tt.HIST


def _mod(kind):
    return tu if kind == "board" else t3


def _host(kind, N, Q, s, seeds, T, X, K, first, rungs=None):
    if kind == "board":
        return tu.host_call(N, s, seeds, T, X, K, first, rungs)
    return t3.host_call(N, Q, s, seeds, T, X, K, first, rungs)


def _restated(kind, N, s, seeds, T, X, K, first, rungs=None):
    """Every ladder through the restatement's ladder_run on the caller's T and X, joined like run_many's result."""
    m, R = _mod(kind), T.shape[1]
    outs = [m.ladder_run(N, s[g: g + R], seeds[g: g + R], T, X, K, first, None if rungs is None else rungs[g: g + R]) for g in range(0, len(s), R)]
    res = {k: np.concatenate([o[k] for o in outs]) for k in m.PER_SLOT + HIST}
    res["pair_accepted"] = np.stack([o["pair_accepted"] for o in outs])
    res["draws"] = [d for o in outs for d in o["draws"]]
    return res


def _plain(kind, N, Q, s, seeds, rows, first):
    """The plain heat-bath host code on a caller's rows uint32[n_sweeps][D], traced."""
    rows = np.ascontiguousarray(rows, dtype=np.uint32)
    return ht.host_with_table(N, s, seeds, rows, first, True) if kind == "board" else ht.host3d(N, Q, s, seeds, rows, rows.shape[0], first)


def _case(kind, i):
    """(N, Q, R, ladders, K, first_sweep, n_sweeps, rung_in given): N and R walk through all their pairs, 2 to 6 ladders (2 at R = 16,
    where the restatement is the slow side), K = 1, 2, 3, first_sweep off a multiple of K, 6 to 10 sweeps, rung_in given in every
    other case."""
    shapes = SHAPES[kind]
    idx = (i + i // 3) % (3 * len(shapes))  # (a stride of its own: the callers walk their tables with periods of 3, 7 and 8)
    (N, Q), R = shapes[idx % len(shapes)], REPLICAS[idx // len(shapes)]
    K = 1 + (i // 2) % 3
    first = K * (i % 4) + (1 + i % (K - 1) if K > 1 else i % 5)
    assert K == 1 or first % K
    return N, Q, R, (2 if R == 16 else 2 + i % 5), K, first, 6 + i % 5, i % 2 == 0


def _inputs(kind, i, seed):
    N, Q, R, ladders, K, first, n_sweeps, given = _case(kind, i)
    n = R * ladders
    s, seeds = tt.placements(kind, N, Q, n, seed + i), abi.seeds_for(4000000000 + 1000 * seed + 37 * i, n)
    rungs = tt.rungs(n, R, seed + i) if given else None
    what = f"{kind} N={N} Q={Q} R={R}, {ladders} ladders, K={K}, {n_sweeps} sweeps from {first}, rung_in={'given' if given else 'default'}"
    return N, Q, R, K, first, n_sweeps, s, seeds, rungs, what


def test_the_cases_cover_every_shape():
    for kind in KINDS:
        cases = [_case(kind, i) for i in range(31)]
        assert {(c[0], c[1]) for c in cases} == set(SHAPES[kind]) and {c[2] for c in cases} == set(REPLICAS), kind
        assert kind == "cube" or {(c[0], c[2]) for c in cases} == {(N, R) for N, _ in SHAPES[kind] for R in REPLICAS}
        assert {c[3] for c in cases} == {2, 3, 4, 5, 6} and {c[4] for c in cases} == {1, 2, 3} and {c[6] for c in cases} == {6, 7, 8, 9, 10}
        assert {c[7] for c in cases} == {True, False} and all(c[4] == 1 or c[5] % c[4] for c in cases)
    assert all(Q in (None, N * N) for N, Q in SHAPES["board"] + SHAPES["cube"][:3]) and all(Q != N * N for N, Q in SHAPES["cube"][3:])


def test_the_tables_are_what_they_say():
    for R in REPLICAS:
        fam, lad = ht.tables(9), tt.ladder_tables(9, R)
        assert set(lad) == {f"same:{f}" for f in tt.FAMILIES} | {"mixed", "mixed_full"}
        D = lad["mixed"].shape[2]
        assert D == 6 and lad["mixed_full"].shape[2] == abi.MAX_HEATBATH_TABLE == 512
        for s in range(9):
            for t in range(R):
                row = fam[tt.FAMILIES[(s + t) % 8]][s]
                np.testing.assert_array_equal(lad["same:" + tt.FAMILIES[(s + t) % 8]][s, t], row)
                np.testing.assert_array_equal(lad["mixed"][s, t, : len(row)], row)
                assert (lad["mixed"][s, t, len(row):] == row[-1]).all()
                if t:
                    np.testing.assert_array_equal(lad["mixed_full"][s, t, :D], lad["mixed"][s, t])
                    assert (lad["mixed_full"][s, t, D:] == row[-1]).all()
        assert (lad["mixed_full"][:, 0] == 1 << 24).all()
        X = tt.swap_tables(4, R, 3)
        assert [X[k].shape[2] for k in tt.SWAPS] == [1, 3, 1, 3, 3, 4096, 5] and (X["max1"] == tt.M).all() and not X["zeros1"].any() and not X["zeros3"].any()
        assert (X["only1"] == [0, tt.M, 0]).all() and (X["clip"] == [0, 0, tt.M]).all() and (X["ramp"][3, R - 2] == np.arange(4096) * 2**20).all()
        assert len(np.unique(X["rand"])) == X["rand"].size and int(X["rand"].max()) > 2**31
    # the closed form of the rungs: R events of odd-even transposition reverse a ladder, whichever parity comes first
    for R in REPLICAS:
        for first in (0, 1):
            h = tt.transposition_rungs(R, np.arange(R), first, R, 1)
            assert (h[:, -1] == R - 1 - np.arange(R)).all() and (np.sort(h, axis=0) == np.arange(R)[:, None]).all() and (np.abs(np.diff(h, axis=1)) <= 1).all()
    assert (tt.transposition_rungs(4, np.arange(4), 0, 4, 3)[:, -1] == [1, 0, 3, 2]).all()  # K = 3: one event, 0, after sweep 2


def test_padding_a_row_with_its_last_entry_changes_nothing():
    """What `mixed` rests on: a distance beyond D - 1 reads the last entry, so a row and the row with its last entry repeated are one
    table.  On mcq_heatbath_host, every family."""
    N, n, T = 5, 6, 6
    s, seeds = qu.random_boards(N, n, 3, over=True), abi.seeds_for(77, n)
    for f in tt.FAMILIES:
        rows = ht.tables(T)[f]
        a, b = ht.host_with_table(N, s, seeds, rows, 2, True), ht.host_with_table(N, s, seeds, tt._padded(rows, rows.shape[1] + 7), 2, True)
        for k in heatbath.FIELDS + ("energy_hist",):
            np.testing.assert_array_equal(a[k], b[k], err_msg=f"{f}: {k}")


@pytest.mark.parametrize("kind", KINDS)
def test_host_code_equals_the_restatement_on_a_callers_tables(kind):
    """Every weight table with the swap tables rand, clip and ramp, and the rows that differ by rung with every swap table: 31 runs per
    entry point.  From the restatement's draws: the table decided both ways, and min(d, DX - 1) read below DX - 1 and at it."""
    weights = tuple(f"same:{f}" for f in tt.FAMILIES) + ("mixed",)
    combos = [(w, x) for w in weights for x in ("rand", "clip", "ramp")] + [("mixed", x) for x in tt.SWAPS if x not in ("rand", "clip", "ramp")]
    assert len(combos) == 31
    m = _mod(kind)
    taken = refused = below = at = 0
    by_swap = {x: [0, 0] for x in tt.SWAPS}
    for i, (w, x) in enumerate(combos):
        N, Q, R, K, first, n_sweeps, s, seeds, rungs, what = _inputs(kind, i, 100)
        T = tt.ladder_tables(n_sweeps, R)[w]
        X = tt.swap_tables(tu.events(first, n_sweeps, K), R, i)[x]
        want = _restated(kind, N, s, seeds, T, X, K, first, rungs)
        got = _host(kind, N, Q, s, seeds, T, X, K, first, rungs)
        m.assert_equal(got, want, f"{what}, {w} x {x}", hist=True)
        DX = X.shape[2]
        for e, t, delta, word, swap in want["draws"]:
            if word is not None:
                taken, refused = taken + swap, refused + (not swap)
                by_swap[x][0 if swap else 1] += 1
                below, at = below + (-delta < DX - 1), at + (-delta >= DX - 1)
    print(f"{kind}: the table took {taken} and refused {refused} pairs; the clamp read below DX - 1 {below} times and at it {at} times; by swap table {by_swap}")
    assert taken >= 10 and refused >= 10 and below >= 10 and at >= 10, (kind, taken, refused, below, at)
    assert min(by_swap["rand"]) > 0 and min(by_swap["clip"]) > 0 and by_swap["ramp"][1] > 0, by_swap  # (ramp: d 2^-12 of the words lie below X[d], few pairs swap)


def test_equal_rows_are_plain_heatbath_chains():
    """same:<family>: every heat-bath output and energy_hist are the plain heat-bath host code's on that family's rows, whatever the
    swap table makes of the rungs -- the tempered staging tied to code that tests/test_heatbath_tables_host.py holds to these families."""
    for kind in KINDS:
        fields = (heatbath.FIELDS if kind == "board" else heatbath.FIELDS_3D) + ("energy_hist",)
        for i, f in enumerate(tt.FAMILIES * 2):
            N, Q, R, K, first, n_sweeps, s, seeds, rungs, what = _inputs(kind, i + 3, 200)
            x = tt.SWAPS[i % len(tt.SWAPS)]
            T = tt.ladder_tables(n_sweeps, R)["same:" + f]
            X = tt.swap_tables(tu.events(first, n_sweeps, K), R, i)[x]
            got = _host(kind, N, Q, s, seeds, T, X, K, first, rungs)
            want = _plain(kind, N, Q, s, seeds, ht.tables(n_sweeps)[f], first)
            for k in fields:
                np.testing.assert_array_equal(np.asarray(got[k]).reshape(np.asarray(want[k]).shape), want[k], err_msg=f"{what}, same:{f} x {x}: {k}")
            assert got["n_exchanges"].sum() > 0, f"{what}, same:{f} x {x}: no rung moved"


def test_without_an_event_each_slot_follows_the_rows_of_its_own_rung():
    """mixed, K beyond the call: slot r is the plain heat-bath host code on the rows T[:, rung_in[r], :] -- not those of its slot, and not
    those of a rung it never had."""
    for kind in KINDS:
        fields = (heatbath.FIELDS if kind == "board" else heatbath.FIELDS_3D) + ("energy_hist",)
        for i in range(6):
            N, Q, R, _, first, n_sweeps, s, seeds, rungs, what = _inputs(kind, i, 300)
            K = first + n_sweeps + 1
            T = tt.ladder_tables(n_sweeps, R)["mixed"]
            got = _host(kind, N, Q, s, seeds, T, tt.swap_tables(1, R, i)["rand"], K, first, rungs)
            assert not got["n_exchanges"].any() and not got["pair_accepted"].any()
            start = np.arange(len(s)) % R if rungs is None else rungs
            assert (got["rung_hist"] == np.asarray(start)[:, None]).all()
            for r in range(len(s)):
                want = _plain(kind, N, Q, s[r: r + 1], seeds[r: r + 1], T[:, start[r], :], first)
                for k in fields:
                    np.testing.assert_array_equal(np.asarray(got[k][r: r + 1]).reshape(np.asarray(want[k]).shape), want[k], err_msg=f"{what}, slot {r}: {k}")
        assert len({tuple(T[0, t]) for t in range(R)}) > 1  # (the rows of a sweep do differ by rung)


# (N, Q, R, ladders, K, first_sweep, sweeps, rung_in given) whose energies spread: weight tables of betas 0.6 .. 1.6 on a ladder
SPREAD = {"board": ((5, None, 4, 6, 1, 3, 8, True), (3, None, 2, 5, 1, 2, 8, False), (5, None, 16, 2, 2, 1, 10, True), (2, None, 4, 6, 3, 1, 9, False),
                    (3, None, 16, 3, 1, 0, 6, True)),
          "cube": ((3, 9, 4, 6, 1, 3, 8, True), (2, 4, 2, 5, 1, 2, 8, False), (4, 16, 16, 2, 2, 1, 10, True), (3, 5, 4, 6, 3, 1, 9, False),
                   (4, 20, 2, 6, 1, 0, 6, True), (2, 3, 16, 3, 1, 4, 7, False))}


def _spread(kind, c, seed, same_seed0=False):
    N, Q, R, ladders, K, first, n_sweeps, given = c
    n = R * ladders
    s, seeds = tt.placements(kind, N, Q, n, seed), abi.seeds_for(3000000000 + seed, n)
    if same_seed0:
        seeds[::R] = seeds[0]
    T = abi.temper_tables(np.linspace(0.6, 1.6, n_sweeps), [float(l) for l in np.linspace(0.5, 2.0, R)], K, first)[0]
    return N, Q, R, K, first, n_sweeps, s, seeds, T, (tt.rungs(n, R, seed) if given else None), f"{kind} N={N} Q={Q} R={R} K={K}, {n_sweeps} sweeps from {first}"


def test_the_swap_follows_delta_under_rows_of_zero_and_the_largest_entry():
    """zeros1, zeros3: a pair swaps iff Delta >= 0; only1 = [0, M, 0]: or Delta = -1; clip = [0, 0, M]: or Delta <= -2, where the clamp
    min(d, DX - 1) lands on the live entry.  Read from the host code's own histories; each class of Delta at least 3 times per entry
    point."""
    for kind in KINDS:
        seen = np.zeros(3, dtype=np.int64)
        for idx, c in enumerate(SPREAD[kind]):
            N, Q, R, K, first, n_sweeps, s, seeds, T, rungs, what = _spread(kind, c, 40 + idx)
            X = tt.swap_tables(tu.events(first, n_sweeps, K), R, idx)
            for name, pred in tt.PREDICATES.items():
                got = _host(kind, N, Q, s, seeds, T, X[name], K, first, rungs)
                tu.check_invariants(got, R, K, first, swap_zero=name.startswith("zeros"))
                counts = tt.assert_swaps_follow(got, R, K, first, pred)
                assert sum(counts) > 0, (what, name)
                seen += counts
        print(f"{kind}: looked-at pairs with Delta >= 0, = -1, <= -2: {tuple(seen)}")
        assert (seen >= 3).all(), (kind, seen)


# (N, Q, R, ladders, K, first_sweep, sweeps, rung_in given) of the aimed rows
AIMED = {"board": ((5, None, 4, 6, 1, 3, 8, True), (12, None, 16, 2, 2, 1, 8, False), (3, None, 2, 6, 1, 2, 10, True)),
         "cube": ((3, 9, 4, 6, 1, 3, 8, True), (6, 30, 16, 2, 2, 1, 8, False), (4, 16, 2, 6, 1, 2, 10, True))}


def test_the_comparison_is_strict_and_reads_the_pairs_own_word():
    """X = the word x the pair draws: `x < X` fails by one, and the run is the run under zeros1.  X = x + 1: it holds by one, and the run
    is the run under max1.  A `<=`, a word of another index or key, or the row of another event or pair moves one of the two."""
    for kind in KINDS:
        m = _mod(kind)
        for idx, c in enumerate(AIMED[kind]):
            N, Q, R, K, first, n_sweeps, s, seeds, T, rungs, what = _spread(kind, c, 60 + idx, same_seed0=True)
            n_events = tu.events(first, n_sweeps, K)
            named = tt.swap_tables(n_events, R, idx)
            runs = {name: _host(kind, N, Q, s, seeds, T, named[name], K, first, rungs) for name in ("zeros1", "max1")}
            for bump, name in ((0, "zeros1"), (1, "max1")):
                X = tt.aimed(seeds[0], R, first // K, n_events, 3 if kind == "board" else 4, bump)
                assert X.shape == (n_events, R - 1, 4) and len(np.unique(X)) == n_events * (R - 1)
                m.assert_equal(_host(kind, N, Q, s, seeds, T, X, K, first, rungs), runs[name], f"{what}: X = x + {bump} against {name}", hist=True)
            assert (runs["zeros1"]["rung_hist"] != runs["max1"]["rung_hist"]).any() and (runs["zeros1"]["state"] != runs["max1"]["state"]).any(), what
            counts = tt.assert_swaps_follow(runs["zeros1"], R, K, first, lambda d: d >= 0)
            print(f"{what}: under zeros1 {counts[1] + counts[2]} looked-at pairs had Delta < 0")
            assert counts[1] + counts[2] >= 10, (what, counts)


def test_rungs_under_the_largest_entry_are_odd_even_transposition():
    """max1: every looked-at pair swaps (its word is not 2^32 - 1), so rung_hist is the closed form, whatever the energies; and after R
    events a ladder that started in order is reversed."""
    for kind in KINDS:
        for i in range(9):
            N, Q, R, K, first, n_sweeps, s, seeds, rungs, what = _inputs(kind, i, 500)
            T = tt.ladder_tables(n_sweeps, R)["mixed"]
            X = tt.swap_tables(tu.events(first, n_sweeps, K), R, i)["max1"]
            got = _host(kind, N, Q, s, seeds, T, X, K, first, rungs)
            start = np.arange(len(s)) % R if rungs is None else rungs
            np.testing.assert_array_equal(got["rung_hist"], tt.transposition_rungs(R, start, first, n_sweeps, K), err_msg=what)
            tu.check_invariants(got, R, K, first)
        N, Q = SHAPES[kind][0]
        for R, first in ((2, 5), (4, 2), (16, 7), (16, 4)):
            n = 3 * R
            s, seeds = tt.placements(kind, N, Q, n, R), abi.seeds_for(R, n)
            got = _host(kind, N, Q, s, seeds, tt.ladder_tables(R, R)["mixed"], tt.swap_tables(R, R, 0)["max1"], 1, first)
            np.testing.assert_array_equal(got["rung_out"], np.tile(np.arange(R)[::-1], 3), err_msg=f"{kind} R={R}: not reversed after R events")
            assert (got["n_exchanges"].reshape(3, R).sum(axis=1) == R * (R - 1)).all() and (got["pair_accepted"].sum(axis=1) == R * (R - 1) // 2).all()


def test_the_word_index_crosses_2_to_the_34():
    """R = 16, K = 1, first_sweep = 2^30 - 3, 6 sweeps: host code = restatement; at least 3 words drawn on either side of 2^34; one word
    on either side recomputed with the oracle's Philox, counter (w / 4 mod 2^32, w >> 34), and the decision with it; and the same ladders
    cut at the crossing, in two calls, against the unbroken call."""
    from oracle import oracle

    for kind, N, Q, key in (("board", 3, None, 3), ("cube", 3, 9, 4)):
        m, R, first, n_sweeps = _mod(kind), tt.WORD_R, tt.WORD_FIRST, tt.WORD_SWEEPS
        s, seeds, T, X, rungs = tt.word_case(kind, N, Q)
        want = _restated(kind, N, s, seeds, T, X, 1, first, rungs)
        got = _host(kind, N, Q, s, seeds, T, X, 1, first, rungs)
        m.assert_equal(got, want, f"{kind} N={N} across 2^34", hist=True)
        drawn = [(e, t, delta, x, swap) for e, t, delta, x, swap in want["draws"] if x is not None]
        sides = (sum(e * R + t < 2**34 for e, t, *_ in drawn), sum(e * R + t >= 2**34 for e, t, *_ in drawn))
        print(f"{kind}: {sides[0]} words drawn below 2^34 and {sides[1]} from it on")
        assert min(sides) >= 3 and sides == tt.word_sides(got), (kind, sides)
        # the draws are in the order of the ladders: the first of each side belongs to the ladder it was found in
        per_ladder = [m.ladder_run(N, s[g: g + R], seeds[g: g + R], T, X, 1, first, rungs[g: g + R])["draws"] for g in range(0, len(s), R)]
        for high in (False, True):
            g, (e, t, delta, x, swap) = next((g, d) for g, ds in enumerate(per_ladder) for d in ds if d[3] is not None and (d[0] * R + d[1] >= 2**34) == high)
            w = e * R + t
            assert (w >> 34) == int(high)
            again = int(oracle.philox_block([(w >> 2) & 0xFFFFFFFF, w >> 34, 0, 0], [int(seeds[g * R]), key])[w & 3])
            assert again == x and swap == (again < int(X[e - first, t, min(-delta, X.shape[2] - 1)])), (kind, w)
            if high:  # and the word is not the one a counter without its high word names
                assert again != int(oracle.philox_block([(w >> 2) & 0xFFFFFFFF, 0, 0, 0], [int(seeds[g * R]), key])[w & 3])
        cut = 3  # the first call ends with event 2^30 - 1, the second starts at sweep 2^30
        a = _host(kind, N, Q, s, seeds, np.ascontiguousarray(T[:cut]), np.ascontiguousarray(X[:cut]), 1, first, rungs)
        b = _host(kind, N, Q, a["state"], seeds, np.ascontiguousarray(T[cut:]), np.ascontiguousarray(X[cut:]), 1, first + cut, a["rung_out"])
        tt.assert_cut_equals_whole(a, b, got, cut, f"{kind} N={N} cut at the crossing")
