"""CPU-only: extremal optimisation in host code (mcq_eo_host) against its NumPy restatement (tests/eo_util.py) on every output, the
history included, at N = 2 .. 13, 16, 17, 24, 25, 31, 32 with both moves, tau = 0, 1.4 and infinity and 0, 1 and N^2 - 1 ranks; the
restatement's Philox against the oracle's; the layout of the mcq_eo block, the LDS formula and the build's fourteenth list; the fifth
table of bindings; every refusal with its text; no iteration; runs cut at three points; first_iter across 2^32; a placement of energy 0
that idles; the all-tied board at N = 2 by closed form; and rank_table against hand values."""
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import mcq_amd
from tests import eo_util as eu

abi = mcq_amd.abi
eo = mcq_amd.eo
_lib = mcq_amd._lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = tuple(range(2, 14)) + (16, 17, 24, 25, 31, 32)
TAUS = (0.0, 1.4, np.inf)


def test_restatement_philox_equals_the_oracles():
    from oracle import oracle

    rs = np.random.RandomState(13)
    for _ in range(40):
        ctr = [int(rs.randint(0, 2**32, dtype=np.uint64)), int(rs.randint(1, 2**31, dtype=np.uint64)), 0, 0]  # a non-zero high word
        key = [int(rs.randint(0, 2**32, dtype=np.uint64)), eu.KEY_WORD]
        assert eu.philox(ctr, key) == [int(x) for x in oracle.philox_block(ctr, key)], (ctr, key)
    assert eu.KEY_WORD == 13
    g = (5 << 32) + 77  # block g: the two halves of g are counter words 0 and 1, key word 1 is 13
    assert eu.block(9, g) == [int(x) for x in oracle.philox_block([77, 5, 0, 0], [9, 13])]
    assert eu.block(9, g) != [int(x) for x in oracle.philox_block([77, 5, 0, 0], [9, 12])]  # not the stream of mcq_nfold3d
    assert eu.block(9, g) != [int(x) for x in oracle.philox_block([77, 5, 0, 0], [9, 7])]   # nor that of mcq_tabu


def test_rank_table_against_hand_values():
    t = eo.rank_table(2, 1.0)  # weights 1, 1/2, 1/3, 1/4 of sum 25/12: P = 12/25, 6/25, 4/25, 3/25
    assert t.dtype == np.uint32 and t.shape == (3,)
    assert [int(x) for x in t] == [(12 << 32) // 25, (18 << 32) // 25, (22 << 32) // 25]
    big = eo.rank_table(32, 1.4).astype(np.int64)
    assert big.shape == (1023,) and (np.diff(big) >= 0).all() and (np.diff(big) > 0).sum() > 1000 and 0 < big[0] < big[-1] < 1 << 32
    assert abs(int(big[0]) / 2.0**32 - 1.0 / float(np.sum(np.arange(1, 1025, dtype=np.float64) ** -1.4))) < 1e-9
    for N in (2, 6, 32):
        assert (eo.rank_table(N, np.inf) == 0xFFFFFFFF).all() and eo.rank_table(N, np.inf).shape == (N * N - 1,)
        uni = eo.rank_table(N, 0.0).astype(np.float64)
        np.testing.assert_allclose(uni / 2.0**32, np.arange(1, N * N) / (N * N), atol=1e-9)
    for bad in (-0.5, np.nan):
        with pytest.raises(ValueError, match="tau"):
            eo.rank_table(6, bad)
    with pytest.raises(ValueError, match="N out of range"):
        eo.rank_table(33, 1.0)
    assert eo.MOVES == ("best", "random")
    with pytest.raises(ValueError, match="Unknown move"):
        eo.eo_states_host(4, eu.random_boards(4, 1, 1), [1], 1, move="worst")


def _tables(N):
    """The rank tables of the comparison at N: none, the first entry of each tau, and each tau's whole table."""
    whole = [eo.rank_table(N, tau) for tau in TAUS]
    return [np.zeros(0, dtype=np.uint32)] + [t[:1] for t in whole] + whole


def _inputs(N):
    n = 3 if N <= 13 else 2
    return eu.random_boards(N, n, 200 + N, over=True), abi.seeds_for(3000000000 + N, n), 40 if N <= 8 else 16 if N <= 17 else 8


@pytest.mark.parametrize("N", SIZES)
def test_host_code_equals_the_restatement(N):
    s, seeds, iters = _inputs(N)
    n = len(s)
    seen = dict.fromkeys(("uphill", "flat", "downhill", "free", "wrapped", "deep", "class_wraps"), 0)
    for move in eo.MOVES:
        for tab in _tables(N):
            got = eo.eo_states_host(N, s, seeds, iters, move=move, rank_cdf=tab, hist=True)
            assert set(got) == set(eo.FIELDS) == set(eu.FIELDS) == set(abi.EO_DTYPES) | {"state", "best_state"}
            assert got["state"].shape == got["best_state"].shape == (n, N * N) and got["energy_hist"].shape == (n, iters + 1)
            for k, dt in abi.EO_DTYPES.items():
                assert got[k].dtype == dt, k
            want = eu.eo_many(N, s, seeds, iters, rank_cdf=tab, move=move)
            eu.assert_equal(got, want, f"N = {N}, {move}, {len(tab)} ranks")
            slim = eo.eo_states_host(N, s, seeds, iters, move=move, rank_cdf=tab)
            assert "energy_hist" not in slim
            eu.assert_equal(slim, want, f"N = {N}, {move}: without the history", fields=[k for k in eu.FIELDS if k in slim])
            for chain in want["trace"]:
                for tr in (tr for tr in chain if tr["moved"]):
                    seen["uphill"] += tr["delta"] > 0
                    seen["flat"] += tr["delta"] == 0
                    seen["downhill"] += tr["delta"] < 0
                    seen["free"] += tr["lam"] == 0
                    seen["wrapped"] += tr["wrapped"]
                    seen["deep"] += tr["j"] > 1
                    seen["class_wraps"] += tr["class_wraps"]
            assert (got["n_moves"] + got["n_idle"] == iters).all()
    print(N, seen)
    assert seen["flat"] > 0 and seen["wrapped"] > 0 and seen["deep"] > 0 and seen["class_wraps"] > 0, seen
    if N >= 3:  # (at N = 2 every two queens attack each other wherever they stand: E = 6 and every move is flat)
        assert seen["uphill"] > 0 and seen["downhill"] > 0, seen
    # the default table is rank_table(N, tau)
    eu.assert_equal(eo.eo_states_host(N, s, seeds, iters, tau=0.7, hist=True), eo.eo_states_host(N, s, seeds, iters, rank_cdf=eo.rank_table(N, 0.7), hist=True), "tau")


def test_struct_layout_lds_formula_build_and_exports():
    fields = [f for f, _ in abi.Eo._fields_]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "mcq.h"\nint main(){printf("%zu %d %d %d %d", sizeof(mcq_eo), MCQ_ABI_VERSION, ' \
        'MCQ_EO_MOVE_BEST, MCQ_EO_MOVE_RANDOM, MCQ_MAX_EO_LDS);' + "".join(f'printf(" %zu", offsetof(mcq_eo, {f}));' for f in fields) + "return 0;}"
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(prog)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")], check=True)
        out = subprocess.run([os.path.join(d, "t")], capture_output=True, text=True, check=True).stdout.split()
    assert int(out[0]) == ctypes.sizeof(abi.Eo) and int(out[1]) == 6 == abi.ABI_VERSION
    assert [int(x) for x in out[2:5]] == [abi.EO_MOVE_BEST, abi.EO_MOVE_RANDOM, abi.MAX_EO_LDS] == [0, 1, 64 * 1024]
    assert [eo.MOVES.index(m) for m in eo.MOVES] == [abi.EO_MOVE_BEST, abi.EO_MOVE_RANDOM]
    assert [int(x) for x in out[5:]] == [getattr(abi.Eo, f).offset for f in fields]
    # the LDS of a chain: the table, the heights, the best placement and N^2 dwords of ranks; below tabu's at every N
    assert abi.eo_lds_bytes(32) == 1024 * (36 + 6) == 43008 and abi.eo_lds_bytes(12) == abi.eo_lds_bytes(9) == 144 * (12 + 6)
    assert abi.eo_lds_bytes(2) == 16 * (4 + 6) and all(abi.eo_lds_bytes(N) <= abi.MAX_EO_LDS for N in range(2, 33))
    assert all(abi.eo_lds_bytes(N) < abi.tabu_lds_bytes(N) for N in range(2, 33))
    b = mcq_amd.build
    assert b.EO_SOURCES == [os.path.join(b.CSRC, "mcq_eo.hip")] and os.path.exists(b.EO_SOURCES[0])
    assert not set(b.EO_SOURCES) & set(b.SOURCES + b.ADDED_SOURCES + b.TEMPER_SOURCES + b.TEMPER3D_SOURCES + b.PAIRS_SOURCES + b.HOP_SOURCES + b.HOP3D_SOURCES
                                      + b.TABU_SOURCES + b.TABU3D_SOURCES + b.RELINK_SOURCES + b.RELINK3D_SOURCES + b.NFOLD_SOURCES + b.NFOLD3D_SOURCES)
    # every function the header names is exported
    header = open(os.path.join(ROOT, "include", "mcq.h")).read()
    named = set(re.findall(r"\b(mcq_eo_\w+)\s*\(", header))
    assert named == {"mcq_eo_last_error", "mcq_eo_device", "mcq_eo_host"}
    L = _lib.lib()
    for name in named:
        assert hasattr(L, name), name


def test_the_fifth_table_of_bindings():
    L = _lib.lib()
    assert tuple(_lib.SEARCH_FEATURES) == ("eo",)
    assert not set(_lib.SEARCH_FEATURES) & (set(_lib.FEATURES) | set(_lib.MORE_FEATURES) | set(_lib.SAMPLER_FEATURES) | set(_lib.SAMPLER3D_FEATURES))
    assert _lib.declared_features() == _lib.bound_features() + list(_lib.SEARCH_FEATURES.values())
    assert _lib.bound_features() == _lib.every_feature() + list(_lib.SAMPLER3D_FEATURES.values())
    assert _lib.SEARCH_FEATURES["eo"] == _lib.Feature(abi.Eo, "eo", ("eo_host", "eo_device"))
    last = L.mcq_eo_last_error
    assert last.restype is ctypes.c_char_p and isinstance(last(), bytes)
    for name in _lib.SEARCH_FEATURES["eo"].entries:
        fn = getattr(L, "mcq_" + name)
        host = name.endswith("_host")
        assert fn.restype is ctypes.c_int and fn.argtypes[0] is ctypes.POINTER(abi.Eo), name
        assert list(fn.argtypes[1:]) == ([] if host else [ctypes.c_void_p]), name
        call = getattr(_lib, name)
        assert callable(call) and call.__name__ == name and "mcq_" + name in call.__doc__ and "abi.Eo" in call.__doc__
        assert (fn(None) if host else fn(None, None)) == abi.EINVAL and b"NULL" in last()
    # a refusal is read from the feature's own buffer, and leaves its neighbours' texts alone
    neighbours = [getattr(L, f"mcq_{p}_last_error")() for p in ("tabu", "nfold", "nfold3d", "relink")]
    with pytest.raises(ValueError) as e:
        _lib.eo_host(eo._block(6, 0, 1, 0, 0, 0))
    assert "n_chains" in str(e.value) and str(e.value) == L.mcq_eo_last_error().decode()
    assert neighbours == [getattr(L, f"mcq_{p}_last_error")() for p in ("tabu", "nfold", "nfold3d", "relink")]


def test_refusals_each_with_its_message():
    L = _lib.lib()
    N, n, iters = 6, 4, 5
    buf, other, spare = (eu.random_boards(N, n, 1) for _ in range(3))
    seeds = abi.seeds_for(1, n)
    ranks = eo.rank_table(N, 1.4)
    falling = ranks.copy()
    falling[7] = falling[6] - 1
    hist = np.zeros((n, iters + 1), dtype=np.int32)

    def block(**kw):
        q = eo._block(N, n, iters, 0, 0, len(ranks))
        q.seeds, q.rank_cdf, q.state_in, q.state_out = seeds.ctypes.data, ranks.ctypes.data, buf.ctypes.data, other.ctypes.data
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    assert L.mcq_eo_host(ctypes.byref(block())) == abi.OK
    cases = [(dict(mode=abi.MODE_FULL3D), "boards only"), (dict(N=1), "N out of range [2, 32]: 1"), (dict(N=33), "N out of range [2, 32]: 33"),
             (dict(n_chains=0), "n_chains out of range"), (dict(n_chains=1 << 31), "n_chains out of range"), (dict(n_iters=-1), "n_iters must be >= 0"),
             (dict(first_iter=-1), "first_iter must be >= 0"), (dict(first_iter=(1 << 63) - 3), "below 2^63"), (dict(move=2), "move must be 0 (best) or 1 (random), got 2"),
             (dict(move=-1), "move must be"), (dict(n_ranks=-1), "n_ranks out of range [0, N^2 - 1 = 35]: -1"), (dict(n_ranks=N * N), "n_ranks out of range"),
             (dict(rank_cdf=None), "rank_cdf is required"), (dict(seeds=None), "seeds is required"), (dict(state_in=None), "state_in is required"),
             (dict(state_out=None), "state_out is required"), (dict(energy_hist=hist.ctypes.data, hist_stride=iters), "hist_stride must be >= n_iters + 1 = 6"),
             (dict(best_state=buf.ctypes.data), "best_state must be distinct"), (dict(best_state=other.ctypes.data), "best_state must be distinct")]
    for kw, text in cases:
        for entry in ("host", "device"):
            q = block(**kw)
            rc = L.mcq_eo_host(ctypes.byref(q)) if entry == "host" else L.mcq_eo_device(ctypes.byref(q), None)
            assert rc == abi.EINVAL and text in L.mcq_eo_last_error().decode(), (kw, entry, L.mcq_eo_last_error())
    # the host entry alone reads the table
    assert L.mcq_eo_host(ctypes.byref(block(rank_cdf=falling.ctypes.data))) == abi.EINVAL and b"rank_cdf must not decrease: entry 7" in L.mcq_eo_last_error()
    with pytest.raises(ValueError, match="must not decrease"):
        eo.eo_states_host(N, buf, seeds, iters, rank_cdf=falling)
    # what is allowed: no rank and no table, state_out = state_in, a best_state of its own, every optional output absent
    q = block(n_ranks=0, rank_cdf=None, state_out=buf.ctypes.data, best_state=spare.ctypes.data)
    before = buf.copy()
    assert L.mcq_eo_host(ctypes.byref(q)) == abi.OK
    want = eu.eo_many(N, before, seeds, iters)
    np.testing.assert_array_equal(buf, want["state"])
    np.testing.assert_array_equal(spare, want["best_state"])
    with pytest.raises(ValueError, match="seeds"):
        eo.eo_states_host(N, before, seeds[:2], iters)
    with pytest.raises(ValueError, match="best_floor"):
        eo.eo_states_host(N, before, seeds, iters, best_floor=[1, 2])
    with pytest.raises(ValueError, match="rank_cdf"):
        eo.eo_states_host(N, before, seeds, iters, rank_cdf=np.zeros((2, 2), dtype=np.uint32))


def test_no_iterations_is_the_recount():
    for N, n in ((5, 4), (13, 2), (32, 1)):
        s, seeds = eu.random_boards(N, n, 9 + N, over=True), abi.seeds_for(1, n)
        got = eo.eo_states_host(N, s, seeds, 0, first_iter=(1 << 40) + 3, hist=True)
        clamped = np.minimum(s, N - 1)
        np.testing.assert_array_equal(got["state"], clamped)
        np.testing.assert_array_equal(got["best_state"], clamped)
        e = np.array([int(eu.badness(N, eu.clamp(N, b)).sum()) // 2 for b in s])
        for k in ("energy_in", "energy_out", "best_energy"):
            np.testing.assert_array_equal(got[k], e, err_msg=k)
        np.testing.assert_array_equal(got["energy_hist"], e[:, None])
        for k in eu.COUNTERS + ("best_iter",):
            assert not got[k].any(), k
        floor = e - np.arange(n, dtype=np.int64) + 1  # above, at and below the recount
        np.testing.assert_array_equal(eo.eo_states_host(N, s, seeds, 0, best_floor=floor.astype(np.int32))["best_energy"], np.minimum(floor, e))


@pytest.mark.parametrize("move", eo.MOVES)
def test_a_cut_run_is_the_unbroken_run(move):
    N, n, iters = 9, 5, 60
    s, seeds = eu.random_boards(N, n, 52, over=True), abi.seeds_for(9, n)
    whole = eo.eo_states_host(N, s, seeds, iters, move=move, first_iter=4, hist=True)
    eu.assert_equal(whole, eu.eo_many(N, s, seeds, iters, rank_cdf=eo.rank_table(N, 1.4), move=move, first_iter=4), "the whole run")
    assert (whole["best_iter"] > 0).any() and whole["n_uphill"].sum() > 0
    for cuts in ((1, iters - 1), (iters - 1, 1), (17, 0, 1, iters - 18)):
        parts = eu.run_cut(eo.eo_states_host, N, s, seeds, cuts, first_iter=4, move=move)
        eu.assert_equal(eu.merge(parts), whole, f"{move}: cut {cuts}")
    # a floor below everything the run reaches: nothing is a new best, and best_state is the input
    low = eo.eo_states_host(N, s, seeds, iters, move=move, best_floor=np.zeros(n, dtype=np.int32))
    assert not low["best_iter"].any() and not low["best_energy"].any()
    np.testing.assert_array_equal(low["best_state"], np.minimum(s, N - 1))


def test_first_iter_across_2_32():
    N, n, iters = 7, 3, 12
    s, seeds = eu.random_boards(N, n, 77), abi.seeds_for(5, n)
    first = (1 << 32) - 5
    tab = eo.rank_table(N, 1.4)
    want = eu.eo_many(N, s, seeds, iters, rank_cdf=tab, first_iter=first)
    got = eo.eo_states_host(N, s, seeds, iters, first_iter=first, hist=True)
    eu.assert_equal(got, want, "first_iter = 2^32 - 5")
    parts = eu.run_cut(eo.eo_states_host, N, s, seeds, (5, 7), first_iter=first)
    eu.assert_equal(eu.merge(parts), want, "cut at 2^32")
    # a counter without its high word would run the iterations 0 .. 6 again behind the first five: not this run
    dropped = eu.eo_many(N, parts[0]["state"], seeds, 7, rank_cdf=tab, first_iter=0, best_floor=parts[0]["best_energy"])
    assert (dropped["energy_hist"] != want["energy_hist"][:, 5:]).any(axis=1).all(), "the high word decides nothing in these runs"


@pytest.mark.parametrize("N", (11, 13))
def test_a_placement_of_energy_0_idles(N):
    k = eu.klarner(N)
    assert not eu.badness(N, eu.clamp(N, k)).any()
    s = np.stack([k, eu.random_boards(N, 1, 3)[0]])
    for move in eo.MOVES:
        got = eo.eo_states_host(N, s, abi.seeds_for(2, 2), 25, move=move, hist=True)
        assert got["n_idle"][0] == 25 and got["n_moves"][0] == 0 and got["n_idle"][1] == 0 and got["n_moves"][1] == 25
        assert not got["energy_hist"][0].any() and got["best_iter"][0] == 0 and got["energy_in"][0] == 0
        np.testing.assert_array_equal(got["state"][0], k)
        np.testing.assert_array_equal(got["best_state"][0], k)
        eu.assert_equal(got, eu.eo_many(N, s, abi.seeds_for(2, 2), 25, rank_cdf=eo.rank_table(N, 1.4), move=move), f"N = {N}, {move}")


def test_the_all_tied_board_by_closed_form():
    """N = 2 with every height 0: every lambda is 3, so the order is the rotation alone and the column moved is (o + j) mod 4."""
    n = 200
    s, seeds = np.zeros((n, 4), dtype=np.uint8), abi.seeds_for(123, n)
    moved = set()
    for i, tab in enumerate((eo.rank_table(2, 0.0), eo.rank_table(2, 1.0), np.zeros(0, dtype=np.uint32), np.zeros(3, dtype=np.uint32))):
        got = eo.eo_states_host(2, s, seeds, 1, rank_cdf=tab)
        assert (got["energy_in"] == 6).all() and (got["n_moves"] == 1).all()
        for r in range(n):
            x = eu.block(int(seeds[r]), 0)
            c = (((x[1] * 4) >> 32) + sum(int(e) <= x[0] for e in tab)) % 4
            want = np.zeros(4, dtype=np.uint8)
            want[c] = 1
            np.testing.assert_array_equal(got["state"][r], want, err_msg=f"chain {r}")
            moved.add((i, c))
        assert (got["energy_out"] == 6).all() and (got["n_flat"] == 1).all()  # at N = 2 every two queens attack each other wherever they stand
    assert len(moved) == 16  # every column under every table
