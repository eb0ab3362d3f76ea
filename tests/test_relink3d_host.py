"""CPU-only: path relinking of full_3d placements in host code (mcq_relink3d_host) against its NumPy restatement (tests/relink3d_util.py)
on every output, the history included: every chain at N = 2 .. 5 with Q = N^2 and at the ragged ends Q = 2, 3, N^3 - 2, N^3 - 1 of
N = 2, 3, 4, two chains at N = 6, chain 0 at N = 13 / Q = 150 and N = 20 / Q = 401; that the compared calls hold ties, wrapped offsets,
rises and falls, winners on and off the moved queen's lines, a P* inside the walk, at the last candidate and none at all, a local
search that moves and one that does not, and results below both endpoints (from the restatement's traces and the host code's outputs,
before a comparison counts); the consequences (a) - (e) of the rule; both repeat flags; walk indices up to 2^63 - 1; every refusal; the
layout of the mcq_relink3d block, the LDS formula at its boundary and the device refusal's text; the second table of bindings; the
build's eleventh list; the 48 images of a placement; the pool."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

import mcq_amd
from tests import quench3d_util as q3
from tests import relink3d_cases as rc
from tests import relink3d_util as ru

abi = mcq_amd.abi
quench = mcq_amd.quench
_lib = mcq_amd._lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (N, Q, chains, few cases, chains restated (None: all))
SQUARE = tuple((N, None, 4, False, None) for N in (2, 3, 4, 5)) + ((6, None, 4, False, 2),)
RAGGED = tuple((N, Q, 3, False, None) for N in (2, 3, 4) for Q in (2, 3, N ** 3 - 2, N ** 3 - 1))
LARGE = ((13, 150, 2, True, 1), (20, 401, 2, True, 1))


def test_the_compared_calls_tie_wrap_rise_fall_and_land_everywhere():
    t = rc.tally([(N, Q, n, few) for N, Q, n, few, rows in SQUARE if rows is None])
    print(rc.check_tally(t, "Q = N^2, N = 2 .. 5"))


def _check_shapes(got, n, N, Q, width):
    assert set(got) == set(quench.FIELDS_RELINK3D)
    assert got["state"].dtype == np.uint8 and got["path_best_state"].dtype == np.uint8 and int(got["state"].max()) < N
    assert got["state"].shape == (n, 3 * Q) and got["energy_hist"].shape == (n, width)
    for k, dt in abi.RELINK3D_DTYPES.items():
        assert got[k].dtype == dt and (k == "energy_hist" or got[k].shape == (n,)), k


@pytest.mark.parametrize("shape", SQUARE + RAGGED + LARGE, ids=lambda s: f"N{s[0]}-Q{s[1]}")
def test_host_code_equals_the_restatement(shape):
    N, Q, n, few, rows = shape
    Qn = rc.queens_of(N, Q)
    for i, (name, s, g, seeds, kw) in enumerate(rc.cases(N, Q, n, few)):
        got = rc.hosted(N, Q, n, few, i)
        _check_shapes(got, n, N, Qn, (kw.get("max_steps") or Qn) + 1)
        ru.assert_equal(got, rc.restated(N, Q, n, few, i, rows), f"N={N} Q={Qn} {name}", rows=None if rows is None else slice(0, rows))
    name, s, g, seeds, kw = rc.cases(N, Q, n, few)[0]
    slim = quench.relink_queens_host(N, s, g, seeds, Q=Q, figures=False, **kw)
    assert set(slim) == {"state"}
    np.testing.assert_array_equal(slim["state"], rc.hosted(N, Q, n, few, 0)["state"])
    only_hist = quench.relink_queens_host(N, s, g, seeds, Q=Q, figures=False, hist=True, **kw)
    assert set(only_hist) == {"state", "energy_hist"}
    np.testing.assert_array_equal(only_hist["energy_hist"], rc.hosted(N, Q, n, few, 0)["energy_hist"])


@pytest.mark.parametrize("N,Q", ((3, None), (4, None), (5, None), (4, 21), (13, 150)))
def test_consequences(N, Q):
    n, few = (4, False) if N <= 5 else (2, True)
    Qn = rc.queens_of(N, Q)
    cs = {c[0]: (i, c) for i, c in enumerate(rc.cases(N, Q, n, few))}
    if True:  # (a) cells(G) = cells(A) in another order: d0 = 0, the call is the quench alone
        i, (name, s, g, seeds, kw) = cs["the guide is the placement, permuted"]
        assert not np.array_equal(np.minimum(s, N - 1), np.minimum(g, N - 1))
        got, ref = rc.hosted(N, Q, n, few, i), quench.quench_queens_host(N, s, Q=Q, conflicts=False)
        assert (got["distance_in"] == 0).all() and (got["n_steps"] == 0).all() and (got["path_best_step"] == 0).all() and (got["flags"] == 0).all()
        for k in ("state", "energy_in", "energy_out", "n_moves", "n_passes"):
            np.testing.assert_array_equal(got[k].astype(np.int64), ref[k].astype(np.int64), err_msg=f"(a) {k}")
        assert (got["energy_hist"] == got["energy_in"][:, None]).all() and (got["path_max_energy"] == got["energy_in"]).all()
        np.testing.assert_array_equal(got["path_best_state"], np.minimum(s, N - 1))
    for name in ("minima", "disjoint", "the guide a candidate", "a cut walk") + (() if few else ("random, bytes >= N",)):
        i, (_, s, g, seeds, kw) = cs[name]
        got = rc.hosted(N, Q, n, few, i)
        rows = np.arange(n)
        if not kw.get("max_steps"):  # (b) the walk ends on the guide's cells
            np.testing.assert_array_equal(got["energy_hist"][rows, got["distance_in"]], [q3.pairwise_energy(N, x) for x in g])
            assert (got["n_steps"] == got["distance_in"]).all()
            if name == "disjoint":
                assert (got["distance_in"] == Qn).all()
        # (c) state_out is a fixed point of L
        again = quench.quench_queens_host(N, got["state"], Q=Q, conflicts=False)
        assert again["n_moves"].sum() == 0 and (again["n_passes"] == 1).all()
        np.testing.assert_array_equal(again["energy_in"], got["energy_out"])
        # (d) path_best_energy is E of path_best_state, and L does not rise
        np.testing.assert_array_equal([q3.pairwise_energy(N, x) for x in got["path_best_state"]], got["path_best_energy"])
        assert (got["energy_out"] <= got["path_best_energy"]).all()
        np.testing.assert_array_equal(got["energy_hist"][rows, got["path_best_step"]], got["path_best_energy"])
        np.testing.assert_array_equal(got["energy_hist"].max(axis=1), got["path_max_energy"])
        # P* is t queens from A, in A's order
        moved = (got["path_best_state"].reshape(n, Qn, 3) != np.minimum(s, N - 1).reshape(n, Qn, 3)).any(axis=2).sum(axis=1)
        np.testing.assert_array_equal(moved, got["path_best_step"])
        # (e) the order of the guide's queens means nothing
        other = quench.relink_queens_host(N, s, rc.permuted(g, 5, Qn), seeds, Q=Q, hist=True, **kw)
        ru.assert_equal(other, got, f"(e) N={N} {name}")


def test_the_window_of_candidates_at_its_edges():
    for N, Q in ((3, None), (5, None), (4, 62)):
        n = 4 if Q is None else 3
        cs = {c[0]: (i, c) for i, c in enumerate(rc.cases(N, Q, n, False))}
        quarter = max(1, rc.room(N, Q) // 4)
        if "one candidate" in cs:
            got = rc.hosted(N, Q, n, False, cs["one candidate"][0])
            assert (got["distance_in"] == 2 * quarter).all() and (got["path_best_step"] == quarter).all()
        i, c = cs["no candidate"]
        got = rc.hosted(N, Q, n, False, i)
        assert (got["distance_in"] == max(1, 2 * quarter - 1)).all() and (got["path_best_step"] == 0).all() and (got["n_steps"] == got["distance_in"]).all()
        np.testing.assert_array_equal(got["path_best_energy"], got["energy_in"])
        np.testing.assert_array_equal(got["path_best_state"], np.minimum(c[1], N - 1))
        got = rc.hosted(N, Q, n, False, cs["the guide a candidate"][0])
        low = got["energy_hist"][:, 1:].astype(np.int64)
        for r in range(n):  # min_dist = 0: every step is a candidate, the guide included; the earliest of the smallest
            d0 = int(got["distance_in"][r])
            if d0:
                assert int(got["path_best_step"][r]) == 1 + int(np.argmin(low[r, :d0]))
        got = rc.hosted(N, Q, n, False, cs["one step, below min_dist"][0])
        assert (got["n_steps"] == np.minimum(1, got["distance_in"])).all() and (got["path_best_step"] == 0).all() and got["energy_hist"].shape[1] == 2


def test_both_repeat_flags():
    N, n = 4, 4
    Q = N * N
    s, g = q3.random_placements(N, n, 3, over=True), q3.random_placements(N, n, 4, over=True)
    s[1, 3:6] = s[1, 0:3]  # A repeated
    g[2, 6:9] = g[2, 0:3]  # G repeated
    s[3, 3:6] = s[3, 0:3]
    g[3, 3:6] = g[3, 0:3]  # both
    seeds = abi.seeds_for(2, n)
    for kw in (dict(), dict(max_steps=5)):
        got = quench.relink_queens_host(N, s, g, seeds, hist=True, **kw)
        np.testing.assert_array_equal(got["flags"], [0, abi.RELINK3D_REPEATED, abi.RELINK3D_GUIDE_REPEATED, abi.RELINK3D_REPEATED | abi.RELINK3D_GUIDE_REPEATED])
        ru.assert_equal(got, ru.relink_many(N, s, g, seeds, **kw), f"repeats {kw}")
        for r in (1, 2, 3):
            e = q3.pairwise_energy(N, s[r])
            assert [int(got[k][r]) for k in ("energy_in", "path_best_energy", "path_max_energy", "energy_out")] == [e] * 4
            assert [int(got[k][r]) for k in ("distance_in", "n_steps", "path_best_step", "n_moves", "n_passes")] == [0] * 5
            assert (got["energy_hist"][r] == e).all() and got["energy_hist"].shape[1] == (kw.get("max_steps") or Q) + 1
            np.testing.assert_array_equal(got["state"][r], np.minimum(s[r], N - 1))
            np.testing.assert_array_equal(got["path_best_state"][r], np.minimum(s[r], N - 1))
        assert got["n_steps"][0] > 0


def test_walks_differ_in_their_tie_orders_and_reach_beyond_32_bits():
    N = 4
    name, s, g, seeds, kw = rc.cases(N)[0]
    walks = (0, 1, (1 << 32) + 1, (5 << 32), (1 << 63) - 1)
    got = {w: quench.relink_queens_host(N, s, g, seeds, walk=w, hist=True, **kw) for w in walks}
    for w in walks:
        want = ru.relink_many(N, s, g, seeds, walk=w, **kw)
        ru.assert_equal(got[w], want, f"walk {w}")
        assert sum(st["ties"] >= 2 for tr in want["trace"] for st in tr) >= 10
    # the same seeds, other tie orders: the low and the high word of walk both reach the counter
    for a, b in ((0, 1), (1, (1 << 32) + 1), (0, 5 << 32)):
        assert not np.array_equal(got[a]["path_best_state"], got[b]["path_best_state"]) or not np.array_equal(got[a]["energy_hist"], got[b]["energy_hist"])


def test_refusals_each_with_its_message():
    L = _lib.lib()
    N, n = 4, 3
    Q = N * N
    buf, guide, other = np.zeros((n, 3 * Q), dtype=np.uint8), np.ones((n, 3 * Q), dtype=np.uint8), np.zeros((n, 3 * Q), dtype=np.uint8)
    buf[:], guide[:] = q3.random_placements(N, n, 1), q3.random_placements(N, n, 2)
    seeds = abi.seeds_for(1, n)
    hist = np.zeros((n, Q + 1), dtype=np.int32)

    def block(**kw):
        q = abi.Relink3d()
        q.N, q.n_queens, q.n_chains, q.max_steps, q.min_dist, q.walk = N, 0, n, 0, 1, 0
        q.seeds, q.state_in, q.guide_in, q.state_out = seeds.ctypes.data, buf.ctypes.data, guide.ctypes.data, other.ctypes.data
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    refused = ((dict(N=1), b"N out of range"), (dict(N=33), b"full_3d path relinking stops at N = 32"), (dict(N=65), b"N out of range"),
               (dict(n_queens=1), b"n_queens out of range"), (dict(n_queens=N ** 3), b"n_queens out of range"), (dict(n_queens=-1), b"n_queens out of range"),
               (dict(n_chains=0), b"n_chains"), (dict(n_chains=-1), b"n_chains"), (dict(n_chains=1 << 31), b"n_chains"),
               (dict(max_steps=-1), b"max_steps out of range"), (dict(max_steps=Q + 1), b"max_steps out of range"),
               (dict(n_queens=5, max_steps=6), b"max_steps out of range"),
               (dict(min_dist=-1), b"min_dist out of range"), (dict(min_dist=Q + 1), b"min_dist out of range"), (dict(walk=-1), b"walk must be"),
               (dict(seeds=None), b"seeds"), (dict(state_in=None), b"state_in is"), (dict(guide_in=None), b"guide_in is"), (dict(state_out=None), b"state_out is"),
               (dict(state_out=guide.ctypes.data), b"distinct from guide_in"),
               (dict(path_best_state=buf.ctypes.data), b"path_best_state"), (dict(path_best_state=guide.ctypes.data), b"path_best_state"),
               (dict(path_best_state=other.ctypes.data), b"path_best_state"),
               (dict(energy_hist=hist.ctypes.data, hist_stride=Q), b"hist_stride"), (dict(energy_hist=hist.ctypes.data, hist_stride=0), b"hist_stride"),
               (dict(energy_hist=hist.ctypes.data, max_steps=5, hist_stride=5), b"hist_stride"))
    before = L.mcq_relink_last_error()
    for kw, msg in refused:
        for fn in (L.mcq_relink3d_host, lambda q: L.mcq_relink3d_device(q, None)):  # refused before any launch: no GPU here
            assert fn(ctypes.byref(block(**kw))) == abi.EINVAL, kw
            assert msg in L.mcq_relink3d_last_error(), (kw, L.mcq_relink3d_last_error())
    assert L.mcq_relink_last_error() == before  # the message is the call's own
    assert L.mcq_relink3d_host(None) == abi.EINVAL and L.mcq_relink3d_device(None, None) == abi.EINVAL and b"NULL" in L.mcq_relink3d_last_error()
    # at the bounds: accepted
    spare = np.zeros_like(buf)
    assert L.mcq_relink3d_host(ctypes.byref(block(max_steps=Q, min_dist=Q))) == abi.OK
    assert L.mcq_relink3d_host(ctypes.byref(block(walk=(1 << 63) - 1))) == abi.OK
    assert L.mcq_relink3d_host(ctypes.byref(block(energy_hist=hist.ctypes.data, hist_stride=Q + 1))) == abi.OK
    assert L.mcq_relink3d_host(ctypes.byref(block(energy_hist=hist.ctypes.data, max_steps=5, hist_stride=6))) == abi.OK
    assert L.mcq_relink3d_host(ctypes.byref(block(hist_stride=0))) == abi.OK  # not read without energy_hist
    assert L.mcq_relink3d_host(ctypes.byref(block(path_best_state=spare.ctypes.data))) == abi.OK
    assert L.mcq_relink3d_host(ctypes.byref(block(state_out=buf.ctypes.data))) == abi.OK  # in place
    with pytest.raises(ValueError, match="N out of range"):
        quench.relink_queens_host(33, np.zeros((2, 3 * 33 * 33), dtype=np.uint8), np.zeros((2, 3 * 33 * 33), dtype=np.uint8), seeds[:2])
    with pytest.raises(ValueError, match="min_dist out of range"):
        quench.relink_queens_host(N, buf, guide, seeds, min_dist=Q + 1)
    with pytest.raises(ValueError, match="n_chains"):
        quench.relink_queens_host(N, np.zeros((0, 3 * Q), dtype=np.uint8), np.zeros((0, 3 * Q), dtype=np.uint8), seeds[:0])
    with pytest.raises(ValueError, match="seeds"):
        quench.relink_queens_host(N, buf, guide, seeds[:2])
    with pytest.raises(ValueError, match="guides must have the shape"):
        quench.relink_queens_host(N, buf, guide[:2], seeds)
    with pytest.raises(ValueError, match="final_state layout"):
        quench.relink_queens_host(N, np.zeros((2, 3 * Q - 1), dtype=np.uint8), np.zeros((2, 3 * Q - 1), dtype=np.uint8), seeds[:2])
    with pytest.raises(ValueError, match="rounds must be"):
        quench.relink_queens_pool_host(N, buf, seeds, 0)
    with pytest.raises(ValueError, match="at least 2"):
        quench.relink_queens_pool_host(N, buf[:1], seeds[:1], 1)


def test_struct_layout_lds_formula_and_build():
    fields = [f for f, _ in abi.Relink3d._fields_]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "mcq.h"\nint main(){printf("%zu %d %d %d %d", sizeof(mcq_relink3d), MCQ_ABI_VERSION, ' \
        'MCQ_MAX_RELINK3D_LDS, MCQ_RELINK3D_REPEATED, MCQ_RELINK3D_GUIDE_REPEATED);' + "".join(f'printf(" %zu", offsetof(mcq_relink3d, {f}));' for f in fields) + "return 0;}"
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(prog)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")], check=True)
        out = subprocess.run([os.path.join(d, "t")], capture_output=True, text=True, check=True).stdout.split()
    assert int(out[0]) == ctypes.sizeof(abi.Relink3d) and int(out[1]) == 6 == abi.ABI_VERSION
    assert [int(x) for x in out[2:5]] == [abi.MAX_RELINK3D_LDS, abi.RELINK3D_REPEATED, abi.RELINK3D_GUIDE_REPEATED]
    assert [int(x) for x in out[5:]] == [getattr(abi.Relink3d, f).offset for f in fields]
    assert set(abi.RELINK3D_DTYPES) | {"state", "path_best_state"} == set(ru.FIELDS) == set(quench.FIELDS_RELINK3D)
    # the formula, part by part, and the figures the header states
    for N, Q in ((2, 4), (12, 144), (19, 361), (20, 400), (32, 1024), (27, 27 ** 3 - 1), (5, 77)):
        C, cpd, D = N ** 3, 4 if N <= 19 else 2, min(Q, N ** 3 - Q)
        parts = (32, -(-C // 32), -(-C // cpd), -(-C // 32), -(-Q // 2), -(-Q // 2), -(-D // 2), -(-D // 2))
        assert abi.relink3d_lds_bytes(N, Q) == 4 * sum(parts), (N, Q)
    assert [abi.relink3d_lds_bytes(N) for N in (12, 32)] == [3440, 82048] and abi.relink3d_lds_bytes(12, 0) == 3440
    assert all(abi.relink3d_lds_bytes(N) <= abi.MAX_RELINK3D_LDS for N in range(2, 33))
    assert abi.relink3d_lds_bytes(32, 11248) == abi.MAX_RELINK3D_LDS < abi.relink3d_lds_bytes(32, 11249)
    assert max(abi.relink3d_lds_bytes(29, Q) for Q in range(2, 29 ** 3)) <= abi.MAX_RELINK3D_LDS < max(abi.relink3d_lds_bytes(30, Q) for Q in range(2, 30 ** 3))
    assert abi.relink3d_lds_bytes(27, 27 ** 3 - 1) <= abi.MAX_RELINK3D_LDS and 27 ** 3 - 1 > 1 << 14
    # the device entry refuses a chain above the LDS before any launch, naming N, Q and the bytes; the host entry runs it
    L = _lib.lib()
    big = q3.random_placements(32, 1, 1, Q=11249)
    q = quench._block_relink3d(32, 11249, 1, 1, 1, 0)
    seeds, out_state = abi.seeds_for(1, 1), np.zeros_like(big)
    q.seeds, q.state_in, q.guide_in, q.state_out = seeds.ctypes.data, big.ctypes.data, big.ctypes.data, out_state.ctypes.data
    assert L.mcq_relink3d_device(ctypes.byref(q), None) == abi.EINVAL
    text = L.mcq_relink3d_last_error().decode()
    assert "N = 32 with n_queens = 11249" in text and f"{abi.relink3d_lds_bytes(32, 11249)} bytes of LDS" in text and str(abi.MAX_RELINK3D_LDS) in text
    b = mcq_amd.build
    assert b.RELINK3D_SOURCES == [os.path.join(b.CSRC, "mcq_relink3d.hip")] and os.path.exists(b.RELINK3D_SOURCES[0])
    assert not set(b.RELINK3D_SOURCES) & set(b.SOURCES + b.ADDED_SOURCES + b.TEMPER_SOURCES + b.TEMPER3D_SOURCES + b.PAIRS_SOURCES + b.HOP_SOURCES + b.HOP3D_SOURCES
                                            + b.TABU_SOURCES + b.TABU3D_SOURCES + b.RELINK_SOURCES)
    for name in ("mcq_relink3d_device", "mcq_relink3d_host", "mcq_relink3d_last_error"):
        assert hasattr(L, name), name


def test_the_second_table_of_bindings():
    L = _lib.lib()
    assert tuple(_lib.MORE_FEATURES) == ("relink3d",) and not set(_lib.MORE_FEATURES) & set(_lib.FEATURES)
    assert _lib.all_features() == list(_lib.FEATURES.values()) + list(_lib.MORE_FEATURES.values())
    for feature, row in _lib.MORE_FEATURES.items():
        last = getattr(L, f"mcq_{row.prefix}_last_error")
        assert last.restype is ctypes.c_char_p and isinstance(last(), bytes)
        assert issubclass(row.struct, ctypes.Structure) and getattr(abi, row.struct.__name__) is row.struct
        assert row.entries[:2] == (feature + "_host", feature + "_device")
        for name in row.entries:
            fn = getattr(L, "mcq_" + name)
            host = name.endswith("_host")
            assert fn.restype is ctypes.c_int and fn.argtypes[0] is ctypes.POINTER(row.struct), name
            assert list(fn.argtypes[1:]) == ([] if host else [ctypes.c_void_p]), name
            call = getattr(_lib, name)
            assert callable(call) and call.__name__ == name and "mcq_" + name in call.__doc__ and "abi." + row.struct.__name__ in call.__doc__
            assert call.__code__.co_varnames[: call.__code__.co_argcount] == (("q",) if host else ("q", "stream"))
            assert (fn(None) if host else fn(None, None)) == abi.EINVAL and b"NULL" in last()
    # a refusal is read from the feature's own buffer, and leaves its neighbours' texts alone
    neighbours = [getattr(L, f"mcq_{p}_last_error")() for p in ("relink", "tabu3d", "hop3d")]
    for block, word in ((quench._block_relink3d(6, 36, 0, 0, 1, 0), "n_chains"), (quench._block_relink3d(1, 1, 4, 0, 1, 0), "N out of range")):
        with pytest.raises(ValueError) as e:
            _lib.relink3d_host(block)
        assert word in str(e.value) and str(e.value) == L.mcq_relink3d_last_error().decode()
    assert neighbours == [getattr(L, f"mcq_{p}_last_error")() for p in ("relink", "tabu3d", "hop3d")]


@pytest.mark.parametrize("N,Q", ((2, 3), (5, None), (6, 50)))
def test_the_48_images_keep_the_energy_and_form_a_group(N, Q):
    Qn = rc.queens_of(N, Q)
    s = q3.random_placements(N, 3, 40 + N, Q=Q)
    imgs = quench.queens_images(N, s, Q=Q)
    assert imgs.shape == (48, 3, 3 * Qn) and imgs.dtype == np.uint8
    np.testing.assert_array_equal(imgs[0], s)
    e = [q3.pairwise_energy(N, x) for x in s]
    for k in range(48):
        assert [q3.pairwise_energy(N, x) for x in imgs[k]] == e, f"image {k}"
    # the numbering: 8 p + 4 f0 + 2 f1 + f2, the axes first and the mirrors behind them
    t = s.reshape(3, Qn, 3)
    np.testing.assert_array_equal(imgs[1].reshape(3, Qn, 3), np.stack([t[..., 0], t[..., 1], N - 1 - t[..., 2]], axis=-1))
    np.testing.assert_array_equal(imgs[4].reshape(3, Qn, 3), np.stack([N - 1 - t[..., 0], t[..., 1], t[..., 2]], axis=-1))
    np.testing.assert_array_equal(imgs[8].reshape(3, Qn, 3), t[..., [0, 2, 1]])
    np.testing.assert_array_equal(imgs[8 * 3 + 2].reshape(3, Qn, 3), np.stack([t[..., 1], N - 1 - t[..., 2], t[..., 0]], axis=-1))
    np.testing.assert_array_equal(imgs[47].reshape(3, Qn, 3), N - 1 - t[..., [2, 1, 0]])
    # a group: an image of an image is an image, and a generic placement has 48 distinct ones
    one = [tuple(x) for x in imgs[:, 0]]
    if N >= 5:
        assert len(set(one)) == 48
    for k in range(48):
        again = quench.queens_images(N, imgs[k], Q=Q)[:, 0]
        assert {tuple(x) for x in again} == set(one), k
    # the nearest image of an image of A is A's cells, at distance 0; the smallest index on ties
    for k in range(48):
        img, idx, dist = quench.nearest_queens_image(N, s, imgs[k], Q=Q)
        if N >= 5:  # (a placement with a symmetry of its own meets its cells at a smaller index too, in another order of the queens)
            np.testing.assert_array_equal(img, s)
        assert [sorted(map(tuple, r.reshape(Qn, 3))) for r in img] == [sorted(map(tuple, r.reshape(Qn, 3))) for r in s]
        assert (dist == 0).all() and idx.dtype == np.int32 and dist.dtype == np.int32
        if N >= 5:
            np.testing.assert_array_equal(quench.queens_images(N, imgs[k], Q=Q)[idx, np.arange(3)], s)
    # the distance is a distance of SETS, and it is the d0 of a relink call
    shuffled = rc.permuted(s, 1, Qn)
    img, idx, dist = quench.nearest_queens_image(N, s, shuffled, Q=Q)
    assert (dist == 0).all() and (idx == 0).all()
    other = q3.random_placements(N, 3, 50 + N, Q=Q)
    far, idx, dist = quench.nearest_queens_image(N, s, other, Q=Q)
    sets = lambda x: [set(map(tuple, r.reshape(Qn, 3))) for r in x]
    brute = np.array([[len(a - b) for a, b in zip(sets(s), sets(im))] for im in quench.queens_images(N, other, Q=Q)])
    np.testing.assert_array_equal(dist, brute.min(axis=0))
    np.testing.assert_array_equal(idx, brute.argmin(axis=0))
    np.testing.assert_array_equal(quench.relink_queens_host(N, s, far, abi.seeds_for(1, 3), Q=Q)["distance_in"], dist)
    with pytest.raises(ValueError, match=">= N"):
        quench.queens_images(N, np.full((1, 3 * Qn), N, dtype=np.uint8), Q=Q)
    with pytest.raises(ValueError, match=">= N"):
        quench.nearest_queens_image(N, np.full((1, 3 * Qn), N, dtype=np.uint8), s[:1], Q=Q)


@pytest.mark.parametrize("align", (True, False))
def test_the_pool_never_rises_and_counts_its_replacements(align):
    N, n, rounds = 4, 24, 3
    s = rc.minima(N, n, 5)
    seeds = abi.seeds_for(9, n)
    e0 = np.array([q3.pairwise_energy(N, x) for x in s])
    prev_state, prev_e = s, e0
    replaced_total = 0
    for k in range(1, rounds + 1):  # the pool behind k rounds is the pool behind k - 1 with one more
        r = quench.relink_queens_pool_host(N, s, seeds, k, align=align, partner_seed=3)
        assert r["n_replaced"].shape == (k,) and r["best_energy"].shape == (k,) and r["energy"].dtype == np.int32
        assert (r["energy"] <= prev_e).all()
        changed = (r["state"] != prev_state).any(axis=1)
        assert int(changed.sum()) == int(r["n_replaced"][-1]) and ((r["energy"] < prev_e) == changed).all()
        np.testing.assert_array_equal([q3.pairwise_energy(N, x) for x in r["state"]], r["energy"])
        assert int(r["best_energy"][-1]) == int(r["energy"].min())
        replaced_total += int(r["n_replaced"][-1])
        prev_state, prev_e = r["state"], r["energy"]
    assert replaced_total > 0  # the pool is not idle on these minima
    # the partners: round k relinks slot r with slot r - s_k
    shifts = np.random.RandomState(3).randint(1, n, size=1)
    one = quench.relink_queens_pool_host(N, s, seeds, 1, align=False, partner_seed=3)
    direct = quench.relink_queens_host(N, s, np.roll(s, int(shifts[0]), axis=0), seeds, min_dist=max(1, N * N // 8), walk=0)
    better = direct["energy_out"] < direct["energy_in"]
    np.testing.assert_array_equal(one["state"], np.where(better[:, None], direct["state"], s))
