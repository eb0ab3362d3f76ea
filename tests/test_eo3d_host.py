"""CPU-only: extremal optimisation of full_3d placements in host code (mcq_eo3d_host) against its NumPy restatement
(tests/eo3d_util.py) on every output, the history included: N = 2 .. 6 with Q = 2, N^2 and N^3 - 1, and N = 12, 13, 19, 20, 32 with
Q = N^2, both moves, tables of 0, 1 and Q - 1 entries at tau = 0, 1.4 and infinity, over-range bytes among the inputs; a coverage gate
from the restatement's traces; the restatement's Philox against the oracle's; the layout of the mcq_eo3d block, the LDS formula, the
build's fifteenth list and the sixth table of bindings; every refusal with its text; no iteration; cut runs; first_iter across 2^32;
a placement of energy 0 that idles; REPEATED inputs; and rank_table with Q against hand values."""
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import mcq_amd
from tests import eo3d_util as eu

abi = mcq_amd.abi
eo = mcq_amd.eo
_lib = mcq_amd._lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAUS = (0.0, 1.4, np.inf)
SMALL = sorted({(N, Q) for N in range(2, 7) for Q in (2, N * N, N ** 3 - 1)})
LARGE = tuple((N, N * N) for N in (12, 13, 19, 20, 32))


def test_restatement_philox_equals_the_oracles():
    from oracle import oracle

    rs = np.random.RandomState(14)
    for _ in range(40):
        ctr = [int(rs.randint(0, 2**32, dtype=np.uint64)), int(rs.randint(1, 2**31, dtype=np.uint64)), 0, 0]  # a non-zero high word
        key = [int(rs.randint(0, 2**32, dtype=np.uint64)), eu.KEY_WORD]
        assert eu.philox(ctr, key) == [int(x) for x in oracle.philox_block(ctr, key)], (ctr, key)
    assert eu.KEY_WORD == 14
    g = (5 << 32) + 77  # block g: the two halves of g are counter words 0 and 1, key word 1 is 14
    assert eu.block(9, g) == [int(x) for x in oracle.philox_block([77, 5, 0, 0], [9, 14])]
    assert eu.block(9, g) != [int(x) for x in oracle.philox_block([77, 5, 0, 0], [9, 13])]  # not the stream of mcq_eo


def test_rank_table_with_q_against_hand_values():
    assert [int(x) for x in eo.rank_table(2, 1.0, Q=2)] == [(2 << 32) // 3]                     # weights 1, 1/2
    assert [int(x) for x in eo.rank_table(3, 1.0, Q=3)] == [(6 << 32) // 11, (9 << 32) // 11]  # weights 1, 1/2, 1/3 of sum 11/6
    t = eo.rank_table(4, 1.4, Q=63)
    assert t.dtype == np.uint32 and t.shape == (62,) and (np.diff(t.astype(np.int64)) > 0).all()
    assert eo.rank_table(32, np.inf, Q=32767).shape == (32766,) and (eo.rank_table(32, np.inf, Q=32767) == 0xFFFFFFFF).all()
    np.testing.assert_allclose(eo.rank_table(5, 0.0, Q=124) / 2.0**32, np.arange(1, 124) / 124, atol=1e-9)
    # unchanged without Q, and Q = N^2 is that table
    for N in (2, 6, 32):
        assert eo.rank_table(N, 1.4).shape == (N * N - 1,)
        np.testing.assert_array_equal(eo.rank_table(N, 1.4), eo.rank_table(N, 1.4, Q=N * N))
    assert [int(x) for x in eo.rank_table(2, 1.0)] == [(12 << 32) // 25, (18 << 32) // 25, (22 << 32) // 25]
    with pytest.raises(ValueError, match="N out of range"):
        eo.rank_table(33, 1.0)
    with pytest.raises(ValueError, match="N out of range"):
        eo.rank_table(33, 1.0, Q=10)
    for bad in (1, 0, 27):
        with pytest.raises(ValueError, match=r"Q out of range \[2, N\^3 - 1 = 26\]"):
            eo.rank_table(3, 1.0, Q=bad)
    with pytest.raises(ValueError, match="tau"):
        eo.rank_table(3, -1.0, Q=5)
    with pytest.raises(ValueError, match="Unknown move"):
        eo.eo_queens_host(4, eu.random_queens(4, 16, 1, 1), [1], 1, move="worst")


def _tables(N, Q):
    """The rank tables of the comparison: none, the first entry of each tau, and each tau's whole table."""
    whole = [eo.rank_table(N, tau, Q) for tau in TAUS]
    return [np.zeros(0, dtype=np.uint32)] + [t[:1] for t in whole] + whole


def _compare(N, Q, n, iters, seed):
    s, seeds = eu.random_queens(N, Q, n, seed, over=True), abi.seeds_for(3000000000 + seed, n)
    if Q == 2:  # (two random queens seldom attack each other: chain 0 holds the ends of a space diagonal, one of them by clamping)
        s[0] = (0, 0, 0, 255, N, 77 + N)
    assert (s >= N).any()
    traces = []
    for move in eo.MOVES:
        for tab in _tables(N, Q):
            got = eo.eo_queens_host(N, s, seeds, iters, Q=Q, move=move, rank_cdf=tab, hist=True)
            assert set(got) == set(eo.FIELDS_QUEENS) == set(eu.FIELDS) == set(abi.EO3D_DTYPES) | {"state", "best_state"}
            assert got["state"].shape == got["best_state"].shape == (n, 3 * Q) and got["energy_hist"].shape == (n, iters + 1)
            for k, dt in abi.EO3D_DTYPES.items():
                assert got[k].dtype == dt, k
            want = eu.eo3d_many(N, s, seeds, iters, Q=Q, rank_cdf=tab, move=move)
            eu.assert_equal(got, want, f"N = {N}, Q = {Q}, {move}, {len(tab)} ranks")
            assert (got["n_moves"] + got["n_idle"] == iters).all() and not got["flags"].any()
            traces += [tr for chain in want["trace"] for tr in chain if tr["moved"]]
    slim = eo.eo_queens_host(N, s, seeds, iters, Q=Q, tau=0.7)  # the default table is rank_table(N, tau, Q); no history
    assert "energy_hist" not in slim
    eu.assert_equal(slim, eo.eo_queens_host(N, s, seeds, iters, Q=Q, rank_cdf=eo.rank_table(N, 0.7, Q), hist=True), "tau", fields=[k for k in eu.FIELDS if k in slim])
    return traces


@pytest.mark.parametrize("N,Q", SMALL)
def test_host_code_equals_the_restatement_small(N, Q):
    traces = _compare(N, Q, 2, 12, 100 * N + Q)
    assert len(traces) > 0


@pytest.mark.parametrize("N,Q", LARGE)
def test_host_code_equals_the_restatement_at_the_edges_of_the_shapes(N, Q):
    traces = _compare(N, Q, 1, 3 if N <= 13 else 2, 7 * N)
    assert any(tr["j"] > 1 for tr in traces) and any(tr["lam"] > 0 for tr in traces)


def test_the_traces_cover_the_rule():
    """The seeds of this file were picked so that the restatement alone meets every case below."""
    seen = dict.fromkeys(("uphill", "flat", "downhill", "free", "deep", "class_wraps", "wrapped", "t_wrapped", "m_first", "m_last"), 0)
    for N, Q, seed in ((3, 9, 1), (3, 25, 2), (4, 16, 3), (5, 25, 4)):
        for tr in _compare(N, Q, 2, 12, seed):
            seen["uphill"] += tr["delta"] > 0
            seen["flat"] += tr["delta"] == 0
            seen["downhill"] += tr["delta"] < 0
            seen["free"] += tr["lam"] == 0
            seen["deep"] += tr["j"] > 1
            seen["class_wraps"] += tr["class_wraps"]
            seen["wrapped"] += tr["wrapped"]
            seen["t_wrapped"] += tr["t_wrapped"]
            seen["m_first"] += tr["F"] > 1 and tr["m"] == 0
            seen["m_last"] += tr["F"] > 1 and tr["m"] == tr["F"] - 1
    print(seen)
    assert all(v > 0 for v in seen.values()), seen


def test_struct_layout_lds_formula_build_and_exports():
    fields = [f for f, _ in abi.Eo3d._fields_]
    assert fields == ["n_queens" if f == "mode" else f for f, _ in abi.Eo._fields_] + ["flags"]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "mcq.h"\nint main(){printf("%zu %d %d %d %d %d", sizeof(mcq_eo3d), MCQ_ABI_VERSION, ' \
        'MCQ_EO3D_MOVE_BEST, MCQ_EO3D_MOVE_RANDOM, MCQ_MAX_EO3D_LDS, MCQ_EO3D_REPEATED);' \
        + "".join(f'printf(" %zu", offsetof(mcq_eo3d, {f}));' for f in fields) + "return 0;}"
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(prog)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")], check=True)
        out = subprocess.run([os.path.join(d, "t")], capture_output=True, text=True, check=True).stdout.split()
    assert int(out[0]) == ctypes.sizeof(abi.Eo3d) and int(out[1]) == 6 == abi.ABI_VERSION
    assert [int(x) for x in out[2:6]] == [abi.EO3D_MOVE_BEST, abi.EO3D_MOVE_RANDOM, abi.MAX_EO3D_LDS, abi.EO3D_REPEATED] == [0, 1, 160 * 1024, 1]
    assert [int(x) for x in out[6:]] == [getattr(abi.Eo3d, f).offset for f in fields]
    # the LDS of a chain: every shape fits, so no shape is refused and none is left to the host code
    for N in range(2, 33):
        for Q in (None, 0, N * N, N ** 3 - 1):
            assert abi.eo3d_lds_bytes(N, Q) <= abi.MAX_EO3D_LDS, (N, Q)
    assert abi.eo3d_lds_bytes(32, 32767) == 135168 + 4 * 480 == 137088 and abi.eo3d_lds_bytes(32) == abi.eo3d_lds_bytes(32, 1024)
    assert abi.eo3d_lds_bytes(12) == 4 * (480 + 432 + 54 + 72) and abi.eo3d_lds_bytes(20, 7999) == 4 * (480 + 4000 + 250 + 4000)
    assert abi.eo3d_lds_bytes(32) < abi.tabu3d_lds_bytes(32)
    b = mcq_amd.build
    assert b.EO3D_SOURCES == [os.path.join(b.CSRC, "mcq_eo3d.hip")] and os.path.exists(b.EO3D_SOURCES[0])
    assert not set(b.EO3D_SOURCES) & set(b.SOURCES + b.ADDED_SOURCES + b.TEMPER_SOURCES + b.TEMPER3D_SOURCES + b.PAIRS_SOURCES + b.HOP_SOURCES + b.HOP3D_SOURCES
                                        + b.TABU_SOURCES + b.TABU3D_SOURCES + b.RELINK_SOURCES + b.RELINK3D_SOURCES + b.NFOLD_SOURCES + b.NFOLD3D_SOURCES
                                        + b.EO_SOURCES)
    # every function the header names is exported, and the Python API is there
    header = open(os.path.join(ROOT, "include", "mcq.h")).read()
    named = set(re.findall(r"\b(mcq_eo3d_\w+)\s*\(", header))
    assert named == {"mcq_eo3d_last_error", "mcq_eo3d_device", "mcq_eo3d_host"}
    L = _lib.lib()
    for name in named:
        assert hasattr(L, name), name
    for name in ("eo_queens_host", "eo_queens_device", "eo_queens", "rank_table", "FIELDS_QUEENS"):
        assert hasattr(mcq_amd.eo, name), name
    assert eo.FIELDS_QUEENS == eo.FIELDS + ("flags",)


def test_the_sixth_table_of_bindings():
    L = _lib.lib()
    assert tuple(_lib.SEARCH3D_FEATURES) == ("eo3d",)
    assert not set(_lib.SEARCH3D_FEATURES) & (set(_lib.FEATURES) | set(_lib.MORE_FEATURES) | set(_lib.SAMPLER_FEATURES) | set(_lib.SAMPLER3D_FEATURES)
                                              | set(_lib.SEARCH_FEATURES))
    assert _lib.linked_features() == _lib.declared_features() + list(_lib.SEARCH3D_FEATURES.values())
    assert _lib.SEARCH3D_FEATURES["eo3d"] == _lib.Feature(abi.Eo3d, "eo3d", ("eo3d_host", "eo3d_device"))
    last = L.mcq_eo3d_last_error
    assert last.restype is ctypes.c_char_p and isinstance(last(), bytes)
    for name in _lib.SEARCH3D_FEATURES["eo3d"].entries:
        fn = getattr(L, "mcq_" + name)
        host = name.endswith("_host")
        assert fn.restype is ctypes.c_int and fn.argtypes[0] is ctypes.POINTER(abi.Eo3d), name
        assert list(fn.argtypes[1:]) == ([] if host else [ctypes.c_void_p]), name
        call = getattr(_lib, name)
        assert callable(call) and call.__name__ == name and "mcq_" + name in call.__doc__ and "abi.Eo3d" in call.__doc__
        assert (fn(None) if host else fn(None, None)) == abi.EINVAL and b"NULL" in last()
    # a refusal is read from the feature's own buffer, and leaves its neighbours' texts alone
    neighbours = [getattr(L, f"mcq_{p}_last_error")() for p in ("eo", "tabu3d", "nfold3d", "relink3d")]
    with pytest.raises(ValueError) as e:
        _lib.eo3d_host(eo._block_queens(6, 0, 0, 1, 0, 0, 0))
    assert "n_chains" in str(e.value) and str(e.value) == L.mcq_eo3d_last_error().decode()
    assert neighbours == [getattr(L, f"mcq_{p}_last_error")() for p in ("eo", "tabu3d", "nfold3d", "relink3d")]


def test_refusals_each_with_its_message():
    L = _lib.lib()
    N, Q, n, iters = 6, 36, 4, 5
    buf, other, spare = (eu.random_queens(N, Q, n, 1) for _ in range(3))
    seeds = abi.seeds_for(1, n)
    ranks = eo.rank_table(N, 1.4, Q)
    falling = ranks.copy()
    falling[7] = falling[6] - 1
    hist = np.zeros((n, iters + 1), dtype=np.int32)

    def block(**kw):
        q = eo._block_queens(N, Q, n, iters, 0, 0, len(ranks))
        q.seeds, q.rank_cdf, q.state_in, q.state_out = seeds.ctypes.data, ranks.ctypes.data, buf.ctypes.data, other.ctypes.data
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    assert L.mcq_eo3d_host(ctypes.byref(block())) == abi.OK
    assert L.mcq_eo3d_host(ctypes.byref(block(n_queens=0))) == abi.OK  # 0 = N^2
    cases = [(dict(N=1), "N out of range [2, 32]: 1"), (dict(N=33), "N out of range [2, 32]: 33 (the full_3d extremal optimisation stops at N = 32"),
             (dict(N=65), "N out of range [2, 32]: 65"), (dict(n_queens=1), "n_queens out of range [2, N^3 - 1 = 215] (0 = N^2): 1"),
             (dict(n_queens=216), "n_queens out of range"), (dict(n_queens=-3), "n_queens out of range"),
             (dict(n_chains=0), "n_chains out of range"), (dict(n_chains=1 << 31), "n_chains out of range"), (dict(n_iters=-1), "n_iters must be >= 0"),
             (dict(first_iter=-1), "first_iter must be >= 0"), (dict(first_iter=(1 << 63) - 3), "below 2^63"), (dict(move=2), "move must be 0 (best) or 1 (random), got 2"),
             (dict(move=-1), "move must be"), (dict(n_ranks=-1), "n_ranks out of range [0, Q - 1 = 35]: -1"), (dict(n_ranks=Q), "n_ranks out of range"),
             (dict(n_queens=20), "n_ranks out of range [0, Q - 1 = 19]: 35"), (dict(rank_cdf=None), "rank_cdf is required"), (dict(seeds=None), "seeds is required"),
             (dict(state_in=None), "state_in is required"), (dict(state_out=None), "state_out is required"),
             (dict(energy_hist=hist.ctypes.data, hist_stride=iters), "hist_stride must be >= n_iters + 1 = 6"),
             (dict(best_state=buf.ctypes.data), "best_state must be distinct"), (dict(best_state=other.ctypes.data), "best_state must be distinct")]
    for kw, text in cases:
        for entry in ("host", "device"):
            q = block(**kw)
            rc = L.mcq_eo3d_host(ctypes.byref(q)) if entry == "host" else L.mcq_eo3d_device(ctypes.byref(q), None)
            assert rc == abi.EINVAL and text in L.mcq_eo3d_last_error().decode(), (kw, entry, L.mcq_eo3d_last_error())
    for entry in (L.mcq_eo3d_host, lambda q: L.mcq_eo3d_device(q, None)):
        assert entry(None) == abi.EINVAL and b"NULL parameter block" in L.mcq_eo3d_last_error()
    # the host entry alone reads the table
    assert L.mcq_eo3d_host(ctypes.byref(block(rank_cdf=falling.ctypes.data))) == abi.EINVAL and b"rank_cdf must not decrease: entry 7" in L.mcq_eo3d_last_error()
    with pytest.raises(ValueError, match="must not decrease"):
        eo.eo_queens_host(N, buf, seeds, iters, rank_cdf=falling)
    # what is allowed: no rank and no table, state_out = state_in, a best_state of its own, every optional output absent
    q = block(n_ranks=0, rank_cdf=None, state_out=buf.ctypes.data, best_state=spare.ctypes.data)
    before = buf.copy()
    assert L.mcq_eo3d_host(ctypes.byref(q)) == abi.OK
    want = eu.eo3d_many(N, before, seeds, iters)
    np.testing.assert_array_equal(buf, want["state"])
    np.testing.assert_array_equal(spare, want["best_state"])
    # the wrappers: the library's text for a shape out of range, their own for the arrays
    with pytest.raises(ValueError, match="N out of range"):
        eo.eo_queens_host(33, np.zeros((1, 3 * 33 * 33), dtype=np.uint8), [1], 1)
    with pytest.raises(ValueError, match="n_queens out of range"):
        eo.eo_queens_host(3, np.zeros((1, 3 * 27), dtype=np.uint8), [1], 1, Q=27)
    with pytest.raises(ValueError, match="states must be"):
        eo.eo_queens_host(N, before[:, :-3], seeds, iters)
    with pytest.raises(ValueError, match="seeds"):
        eo.eo_queens_host(N, before, seeds[:2], iters)
    with pytest.raises(ValueError, match="best_floor"):
        eo.eo_queens_host(N, before, seeds, iters, best_floor=[1, 2])
    with pytest.raises(ValueError, match="rank_cdf"):
        eo.eo_queens_host(N, before, seeds, iters, rank_cdf=np.zeros((2, 2), dtype=np.uint32))


def test_no_iterations_is_the_recount():
    for N, Q, n in ((5, 25, 4), (4, 63, 3), (13, 169, 2), (32, 1024, 1)):
        s, seeds = eu.random_queens(N, Q, n, 9 + N, over=True), abi.seeds_for(1, n)
        got = eo.eo_queens_host(N, s, seeds, 0, Q=Q, first_iter=(1 << 40) + 3, hist=True)
        clamped = np.minimum(s, N - 1)
        np.testing.assert_array_equal(got["state"], clamped)
        np.testing.assert_array_equal(got["best_state"], clamped)
        e = np.array([int(eu.badness(eu.clamp(N, p)).sum()) // 2 for p in s])
        for k in ("energy_in", "energy_out", "best_energy"):
            np.testing.assert_array_equal(got[k], e, err_msg=k)
        np.testing.assert_array_equal(got["energy_hist"], e[:, None])
        for k in eu.COUNTERS + ("best_iter", "flags"):
            assert not got[k].any(), k
        floor = e - np.arange(n, dtype=np.int64) + 1  # above, at and below the recount
        np.testing.assert_array_equal(eo.eo_queens_host(N, s, seeds, 0, Q=Q, best_floor=floor.astype(np.int32))["best_energy"], np.minimum(floor, e))


@pytest.mark.parametrize("move", eo.MOVES)
def test_a_cut_run_is_the_unbroken_run(move):
    N, Q, n, iters = 5, 30, 4, 40
    s, seeds = eu.random_queens(N, Q, n, 52, over=True), abi.seeds_for(9, n)
    whole = eo.eo_queens_host(N, s, seeds, iters, Q=Q, move=move, first_iter=4, hist=True)
    eu.assert_equal(whole, eu.eo3d_many(N, s, seeds, iters, Q=Q, rank_cdf=eo.rank_table(N, 1.4, Q), move=move, first_iter=4), "the whole run")
    assert (whole["best_iter"] > 0).any() and whole["n_uphill"].sum() > 0
    for cuts in ((1, iters - 1), (iters - 1, 1), (17, 0, 1, iters - 18)):
        parts = eu.run_cut(eo.eo_queens_host, N, s, seeds, cuts, first_iter=4, move=move, Q=Q)
        eu.assert_equal(eu.merge(parts), whole, f"{move}: cut {cuts}")
    # a floor below everything the run reaches: nothing is a new best, and best_state is the input
    low = eo.eo_queens_host(N, s, seeds, iters, Q=Q, move=move, best_floor=np.zeros(n, dtype=np.int32))
    assert not low["best_iter"].any() and not low["best_energy"].any()
    np.testing.assert_array_equal(low["best_state"], np.minimum(s, N - 1))


def test_first_iter_across_2_32():
    N, Q, n, iters = 4, 16, 3, 12
    s, seeds = eu.random_queens(N, Q, n, 77), abi.seeds_for(5, n)
    first = (1 << 32) - 5
    tab = eo.rank_table(N, 1.4, Q)
    want = eu.eo3d_many(N, s, seeds, iters, rank_cdf=tab, first_iter=first)
    got = eo.eo_queens_host(N, s, seeds, iters, first_iter=first, hist=True)
    eu.assert_equal(got, want, "first_iter = 2^32 - 5")
    parts = eu.run_cut(eo.eo_queens_host, N, s, seeds, (5, 7), first_iter=first)
    eu.assert_equal(eu.merge(parts), want, "cut at 2^32")
    # a counter without its high word would run the iterations 0 .. 6 again behind the first five: not this run
    dropped = eu.eo3d_many(N, parts[0]["state"], seeds, 7, rank_cdf=tab, first_iter=0, best_floor=parts[0]["best_energy"])
    assert (dropped["energy_hist"] != want["energy_hist"][:, 5:]).any(axis=1).all(), "the high word decides nothing in these runs"


def test_a_placement_of_energy_0_idles():
    N, Q = 4, 2
    calm = np.array([0, 0, 0, 1, 2, 3], dtype=np.uint8)  # two queens that do not attack each other
    assert not eu.badness(eu.clamp(N, calm)).any()
    s = np.stack([calm, np.array([0, 0, 0, 1, 1, 1], dtype=np.uint8)])
    for move in eo.MOVES:
        got = eo.eo_queens_host(N, s, abi.seeds_for(2, 2), 25, Q=Q, move=move, hist=True)
        assert got["n_idle"][0] == 25 and got["n_moves"][0] == 0 and got["n_moves"][1] > 0 and got["n_moves"][1] + got["n_idle"][1] == 25
        assert not got["energy_hist"][0].any() and got["best_iter"][0] == 0 and got["energy_in"][0] == 0 and got["energy_in"][1] == 1
        np.testing.assert_array_equal(got["state"][0], calm)
        np.testing.assert_array_equal(got["best_state"][0], calm)
        eu.assert_equal(got, eu.eo3d_many(N, s, abi.seeds_for(2, 2), 25, Q=Q, rank_cdf=eo.rank_table(N, 1.4, Q), move=move), f"{move}")


def test_a_repeated_input_is_handed_back_unmoved():
    N, Q, n, iters = 5, 25, 3, 6
    s = eu.random_queens(N, Q, n, 31)
    s[0, 3:6] = s[0, 0:3]          # two queens in one cell
    s[2, 6:9] = (4, 4, 200)         # ... after clamping only
    s[2, 9:12] = (4, 4, 4)
    seeds = abi.seeds_for(8, n)
    for move in eo.MOVES:
        got = eo.eo_queens_host(N, s, seeds, iters, move=move, best_floor=np.zeros(n, dtype=np.int32), hist=True)
        want = eu.eo3d_many(N, s, seeds, iters, rank_cdf=eo.rank_table(N, 1.4, Q), move=move, best_floor=np.zeros(n, dtype=np.int32))
        eu.assert_equal(got, want, f"{move}")
        assert list(got["flags"]) == [abi.EO3D_REPEATED, 0, abi.EO3D_REPEATED] == [eu.REPEATED, 0, eu.REPEATED]
        for r in (0, 2):
            np.testing.assert_array_equal(got["state"][r], np.minimum(s[r], N - 1))
            np.testing.assert_array_equal(got["best_state"][r], np.minimum(s[r], N - 1))
            assert got["energy_in"][r] == got["energy_out"][r] == got["best_energy"][r] > 0 and (got["energy_hist"][r] == got["energy_in"][r]).all()
            assert not any(got[k][r] for k in eu.COUNTERS + ("best_iter",))
        assert got["n_moves"][1] == iters and got["best_energy"][1] == 0  # the floor is looked at where the input is no such placement


def test_the_single_free_cell_is_the_target_of_both_moves():
    for N in (3, 5):
        hole = 7
        s = eu.cube_without(N, [hole])[None]
        for move in eo.MOVES:
            got = eo.eo_queens_host(N, s, [5], 3, Q=N ** 3 - 1, move=move, hist=True)
            want = eu.eo3d_many(N, s, [5], 3, Q=N ** 3 - 1, rank_cdf=eo.rank_table(N, 1.4, N ** 3 - 1), move=move)
            eu.assert_equal(got, want, f"N = {N}, {move}")
            assert want["trace"][0][0]["t"] == hole and all(tr["m"] == 0 and tr["F"] == 1 for tr in want["trace"][0])
