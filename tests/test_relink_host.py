"""CPU-only: path relinking in host code (mcq_relink_host) against its NumPy restatement (tests/relink_util.py) on every output, the
history included, under both local searches: every chain at N = 2 .. 12, chain 0 at N = 13 .. 32; that the compared calls hold ties
whose winner is not the smallest column, wrapped offsets, rises and falls, a P* inside the walk, at the last candidate and none at all,
a local search that moves and one that does not, pair moves, and results below both endpoints (from the restatement's traces and the
host code's outputs, before a comparison counts); the consequences (a) - (d) of the rule; the window of candidates at its edges; two
walks with different tie orders and a walk index beyond 2^32; every refusal; the layout of the mcq_relink block and the build's tenth
list; the 16 images of a board; the pool."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

import mcq_amd
from tests import quench_util as qu
from tests import relink_cases as rc
from tests import relink_util as ru

abi = mcq_amd.abi
quench = mcq_amd.quench
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("search", rc.SEARCHES)
@pytest.mark.parametrize("grp", (4, 8, 12, 16, 24, 32))
def test_the_compared_calls_tie_wrap_rise_fall_and_land_everywhere(grp, search):
    print(grp, search, rc.coverage(search, grp).check(grp, pairs=search == "pairs"))


def _check_shapes(got, n, N, width):
    assert set(got) == set(quench.FIELDS_RELINK)
    assert got["state"].dtype == np.uint8 and got["path_best_state"].dtype == np.uint8 and int(got["state"].max()) < N
    assert got["energy_hist"].shape == (n, width)
    for k, dt in abi.RELINK_DTYPES.items():
        assert got[k].dtype == dt and (k == "energy_hist" or got[k].shape == (n,)), k


@pytest.mark.parametrize("search", rc.SEARCHES)
@pytest.mark.parametrize("N", rc.ALL_N)
def test_host_code_equals_the_restatement(N, search):
    rc.coverage(search, rc.group(N)).check(rc.group(N), pairs=search == "pairs")
    rows = None if N in rc.FULL else slice(0, 1)
    for i, (name, s, g, seeds, kw, runs) in enumerate(rc.cases(N)):
        got = rc.hosted(N, i, search)
        _check_shapes(got, s.shape[0], N, (kw.get("max_steps") or N * N) + 1)
        if runs:
            ru.assert_equal(got, rc.restated(N, i, search), f"N={N} {name} {search}", rows=rows)
    name, s, g, seeds, kw, runs = rc.cases(N)[0]
    slim = quench.relink_host(N, s, g, seeds, local_search=search, figures=False, **kw)
    assert set(slim) == {"state"}
    np.testing.assert_array_equal(slim["state"], rc.hosted(N, 0, search)["state"])
    only_hist = quench.relink_host(N, s, g, seeds, local_search=search, figures=False, hist=True, **kw)
    assert set(only_hist) == {"state", "energy_hist"}
    np.testing.assert_array_equal(only_hist["energy_hist"], rc.hosted(N, 0, search)["energy_hist"])


@pytest.mark.parametrize("N", (4, 9, 12, 17, 32))
def test_consequences(N):
    cases = {c[0]: (i, c) for i, c in enumerate(rc.cases(N))}
    # (a) d0 = 0 is L alone
    i, (name, s, g, seeds, kw, runs) = cases["the guide is the placement"]
    for search, ref in (("pairs", quench.quench_pairs_host(N, s, conflicts=False)), ("single", quench.quench_states_host(N, s, conflicts=False))):
        got = rc.hosted(N, i, search)
        assert (got["distance_in"] == 0).all() and (got["n_steps"] == 0).all() and (got["path_best_step"] == 0).all()
        for k in ("state", "energy_in", "energy_out", "n_moves") + (("n_pair_moves",) if search == "pairs" else ()):
            np.testing.assert_array_equal(got[k].astype(np.int64), ref[k].astype(np.int64), err_msg=f"(a) {search} {k}")
        assert (got["energy_hist"] == got["energy_in"][:, None]).all() and (got["path_max_energy"] == got["energy_in"]).all()
        np.testing.assert_array_equal(got["path_best_state"], np.minimum(s, N - 1))
    assert (rc.hosted(N, i, "single")["n_pair_moves"] == 0).all() and rc.hosted(N, i, "pairs")["n_moves"].sum() > 0
    for name in ("minima", "every column differs", "random, bytes >= N", "minima, the guide a candidate"):
        i, (_, s, g, seeds, kw, runs) = cases[name]
        for search in rc.SEARCHES:
            got = rc.hosted(N, i, search)
            n = np.arange(s.shape[0])
            # (b) with max_steps = 0 the walk ends on the guide
            if not kw.get("max_steps"):
                back = quench.relink_host(N, g, s, seeds, local_search=search, **kw)
                np.testing.assert_array_equal(got["energy_hist"][n, got["distance_in"]], back["energy_in"])
                np.testing.assert_array_equal(got["distance_in"], back["distance_in"])
                assert (got["n_steps"] == got["distance_in"]).all()
                if name == "every column differs":
                    assert (got["distance_in"] == N * N).all()
            # (c) state_out is a fixed point of L
            again = quench.quench_pairs_host(N, got["state"], conflicts=False) if search == "pairs" else quench.quench_states_host(N, got["state"], conflicts=False)
            assert again["n_moves"].sum() == 0 and again.get("n_pair_moves", np.zeros(1)).sum() == 0
            np.testing.assert_array_equal(again["energy_in"], got["energy_out"])
            # (d) path_best_energy is E of path_best_state, and L does not rise
            recount = quench.quench_states_host(N, got["path_best_state"], max_passes=1, conflicts=False)["energy_in"]
            np.testing.assert_array_equal(recount, got["path_best_energy"])
            assert (got["energy_out"] <= got["path_best_energy"]).all()
            np.testing.assert_array_equal(got["energy_hist"][n, got["path_best_step"]], got["path_best_energy"])
            np.testing.assert_array_equal(got["energy_hist"].max(axis=1), got["path_max_energy"])
            # P* is t columns from A and d0 - t from the guide
            np.testing.assert_array_equal((got["path_best_state"] != np.minimum(s, N - 1)).sum(axis=1), got["path_best_step"])
            np.testing.assert_array_equal((got["path_best_state"] != np.minimum(g, N - 1)).sum(axis=1), got["distance_in"] - got["path_best_step"])


@pytest.mark.parametrize("N", (2, 4, 12, 32))
def test_the_window_of_candidates_at_its_edges(N):
    cases = {c[0]: (i, c) for i, c in enumerate(rc.cases(N))}
    quarter = rc.edge_dist(N)
    i, c = cases["one candidate"]
    got = rc.hosted(N, i, "pairs")
    assert (got["distance_in"] == 2 * quarter).all() and (got["path_best_step"] == quarter).all()
    i, c = cases["no candidate"]
    got = rc.hosted(N, i, "pairs")
    assert (got["distance_in"] == 2 * quarter - 1).all() and (got["path_best_step"] == 0).all() and (got["n_steps"] == 2 * quarter - 1).all()
    np.testing.assert_array_equal(got["path_best_energy"], got["energy_in"])
    np.testing.assert_array_equal(got["path_best_state"], np.minimum(c[1], N - 1))
    i, c = cases["minima, the guide a candidate"]
    got = rc.hosted(N, i, "pairs")
    low = got["energy_hist"][:, 1:].astype(np.int64)
    for r in range(low.shape[0]):  # min_dist = 0: every step is a candidate, the guide included; the earliest of the smallest
        d0 = int(got["distance_in"][r])
        if d0:
            assert int(got["path_best_step"][r]) == 1 + int(np.argmin(low[r, :d0]))
    i, c = cases["one step, below min_dist"]
    got = rc.hosted(N, i, "pairs")
    assert (got["n_steps"] == np.minimum(1, got["distance_in"])).all() and (got["path_best_step"] == 0).all() and got["energy_hist"].shape[1] == 2


def test_walks_differ_in_their_tie_orders_and_reach_beyond_32_bits():
    N = 8
    name, s, g, seeds, kw, runs = rc.cases(N)[0]
    walks = (0, 1, (1 << 32) + 1, (5 << 32), (1 << 63) - 1)
    got = {w: quench.relink_host(N, s, g, seeds, walk=w, hist=True, **kw) for w in walks}
    for w in walks:
        want = ru.relink_many(N, s, g, seeds, walk=w, **kw)
        ru.assert_equal(got[w], want, f"walk {w}")
        assert sum(st["ties"] >= 2 for tr in want["trace"] for st in tr) >= 10
    # the same seeds, other tie orders: the low and the high word of walk both reach the counter
    for a, b in ((0, 1), (1, (1 << 32) + 1), (0, 5 << 32)):
        assert not np.array_equal(got[a]["path_best_state"], got[b]["path_best_state"]) or not np.array_equal(got[a]["energy_hist"], got[b]["energy_hist"])


def test_refusals_each_with_its_message():
    L = mcq_amd._lib.lib()
    N, n = 6, 4
    buf, guide, other = np.zeros((n, N * N), dtype=np.uint8), np.ones((n, N * N), dtype=np.uint8), np.zeros((n, N * N), dtype=np.uint8)
    seeds = abi.seeds_for(1, n)
    hist = np.zeros((n, N * N + 1), dtype=np.int32)

    def block(**kw):
        q = abi.Relink()
        q.N, q.mode, q.n_chains, q.max_steps, q.min_dist, q.local_search, q.walk = N, abi.MODE_BOARD, n, 0, 1, abi.HOP_PAIRS, 0
        q.seeds, q.state_in, q.guide_in, q.state_out = seeds.ctypes.data, buf.ctypes.data, guide.ctypes.data, other.ctypes.data
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    refused = ((dict(mode=abi.MODE_FULL3D), b"mode"), (dict(mode=7), b"mode"), (dict(N=1), b"N out of range"), (dict(N=33), b"N out of range"),
               (dict(n_chains=0), b"n_chains"), (dict(n_chains=-1), b"n_chains"), (dict(n_chains=1 << 31), b"n_chains"),
               (dict(max_steps=-1), b"max_steps out of range"), (dict(max_steps=N * N + 1), b"max_steps out of range"),
               (dict(min_dist=-1), b"min_dist out of range"), (dict(min_dist=N * N + 1), b"min_dist out of range"),
               (dict(local_search=2), b"local_search"), (dict(local_search=-1), b"local_search"), (dict(walk=-1), b"walk must be"),
               (dict(seeds=None), b"seeds"), (dict(state_in=None), b"state_in is"), (dict(guide_in=None), b"guide_in is"), (dict(state_out=None), b"state_out is"),
               (dict(state_out=guide.ctypes.data), b"distinct from guide_in"),
               (dict(path_best_state=buf.ctypes.data), b"path_best_state"), (dict(path_best_state=guide.ctypes.data), b"path_best_state"),
               (dict(path_best_state=other.ctypes.data), b"path_best_state"),
               (dict(energy_hist=hist.ctypes.data, hist_stride=N * N), b"hist_stride"), (dict(energy_hist=hist.ctypes.data, hist_stride=0), b"hist_stride"),
               (dict(energy_hist=hist.ctypes.data, max_steps=5, hist_stride=5), b"hist_stride"))
    before = L.mcq_tabu_last_error()
    for kw, msg in refused:
        for fn in (L.mcq_relink_host, lambda q: L.mcq_relink_device(q, None)):  # refused before any launch: no GPU here
            assert fn(ctypes.byref(block(**kw))) == abi.EINVAL, kw
            assert msg in L.mcq_relink_last_error(), (kw, L.mcq_relink_last_error())
    assert L.mcq_tabu_last_error() == before  # the message is the call's own
    assert L.mcq_relink_host(None) == abi.EINVAL and L.mcq_relink_device(None, None) == abi.EINVAL and b"NULL" in L.mcq_relink_last_error()
    # at the bounds: accepted
    spare = np.zeros_like(buf)
    assert L.mcq_relink_host(ctypes.byref(block(max_steps=N * N, min_dist=N * N))) == abi.OK
    assert L.mcq_relink_host(ctypes.byref(block(walk=(1 << 63) - 1))) == abi.OK
    assert L.mcq_relink_host(ctypes.byref(block(energy_hist=hist.ctypes.data, hist_stride=N * N + 1))) == abi.OK
    assert L.mcq_relink_host(ctypes.byref(block(energy_hist=hist.ctypes.data, max_steps=5, hist_stride=6))) == abi.OK
    assert L.mcq_relink_host(ctypes.byref(block(hist_stride=0))) == abi.OK  # not read without energy_hist
    assert L.mcq_relink_host(ctypes.byref(block(path_best_state=spare.ctypes.data))) == abi.OK
    assert L.mcq_relink_host(ctypes.byref(block(state_out=buf.ctypes.data))) == abi.OK  # in place
    with pytest.raises(ValueError, match="N out of range"):
        quench.relink_host(33, np.zeros((2, 33 * 33), dtype=np.uint8), np.zeros((2, 33 * 33), dtype=np.uint8), seeds[:2])
    with pytest.raises(ValueError, match="min_dist out of range"):
        quench.relink_host(6, buf, guide, seeds, min_dist=37)
    with pytest.raises(ValueError, match="n_chains"):
        quench.relink_host(6, np.zeros((0, 36), dtype=np.uint8), np.zeros((0, 36), dtype=np.uint8), seeds[:0])
    with pytest.raises(ValueError, match="seeds"):
        quench.relink_host(6, buf, guide, seeds[:3])
    with pytest.raises(ValueError, match="guides must have the shape"):
        quench.relink_host(6, buf, guide[:3], seeds)
    with pytest.raises(ValueError, match="local_search"):
        quench.relink_host(6, buf, guide, seeds, local_search="triples")
    with pytest.raises(ValueError, match="final_state layout"):
        quench.relink_host(6, np.zeros((2, 35), dtype=np.uint8), np.zeros((2, 35), dtype=np.uint8), seeds[:2])
    with pytest.raises(ValueError, match="rounds must be"):
        quench.relink_pool_host(6, buf, seeds, 0)
    with pytest.raises(ValueError, match="at least 2"):
        quench.relink_pool_host(6, buf[:1], seeds[:1], 1)


def test_struct_layout_and_build():
    fields = [f for f, _ in abi.Relink._fields_]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "mcq.h"\nint main(){printf("%zu %d %d %d %d", sizeof(mcq_relink), MCQ_ABI_VERSION, ' \
        'MCQ_MAX_RELINK_LDS, MCQ_HOP_SINGLE, MCQ_HOP_PAIRS);' + "".join(f'printf(" %zu", offsetof(mcq_relink, {f}));' for f in fields) + "return 0;}"
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(prog)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")], check=True)
        out = subprocess.run([os.path.join(d, "t")], capture_output=True, text=True, check=True).stdout.split()
    assert int(out[0]) == ctypes.sizeof(abi.Relink) and int(out[1]) == 6 == abi.ABI_VERSION
    assert [int(x) for x in out[2:5]] == [abi.MAX_RELINK_LDS, abi.HOP_SINGLE, abi.HOP_PAIRS]
    assert [int(x) for x in out[5:]] == [getattr(abi.Relink, f).offset for f in fields]
    assert set(abi.RELINK_DTYPES) | {"state", "path_best_state"} == set(ru.FIELDS) | {"energy_hist"} == set(quench.FIELDS_RELINK)
    assert [abi.relink_lds_bytes(N) for N in (2, 4, 5, 8, 12, 16, 17, 24, 32)] == [240, 240, 1472, 1472, 3312, 7936, 22464, 22464, 48128]
    assert [abi.relink_lds_bytes(N, pairs=False) for N in (4, 32)] == [112, 39936] and abi.relink_lds_bytes(32) <= abi.MAX_RELINK_LDS
    b = mcq_amd.build
    assert b.RELINK_SOURCES == [os.path.join(b.CSRC, "mcq_relink.hip")] and os.path.exists(b.RELINK_SOURCES[0])
    assert not set(b.RELINK_SOURCES) & set(b.SOURCES + b.ADDED_SOURCES + b.TEMPER_SOURCES + b.TEMPER3D_SOURCES + b.PAIRS_SOURCES + b.HOP_SOURCES + b.HOP3D_SOURCES
                                          + b.TABU_SOURCES + b.TABU3D_SOURCES)
    L = mcq_amd._lib.lib()
    for name in ("mcq_relink_device", "mcq_relink_host", "mcq_relink_last_error"):
        assert hasattr(L, name), name


@pytest.mark.parametrize("N", (2, 5, 8))
def test_the_sixteen_images_keep_the_energy_and_form_a_group(N):
    s = qu.random_boards(N, 3, 40 + N)
    imgs = quench.board_images(N, s)
    assert imgs.shape == (16, 3, N * N) and imgs.dtype == np.uint8
    np.testing.assert_array_equal(imgs[0], s)
    e = quench.quench_states_host(N, s, max_passes=1, conflicts=False)["energy_in"]
    for k in range(16):
        np.testing.assert_array_equal(quench.quench_states_host(N, imgs[k], max_passes=1, conflicts=False)["energy_in"], e, err_msg=f"image {k}")
    # the numbering: 8 f + 4 m + r
    b = s.reshape(3, N, N)
    np.testing.assert_array_equal(imgs[8], (N - 1 - s))
    np.testing.assert_array_equal(imgs[4].reshape(3, N, N), b.swapaxes(1, 2))
    np.testing.assert_array_equal(imgs[1].reshape(3, N, N), np.rot90(b, 1, axes=(1, 2)))
    np.testing.assert_array_equal(imgs[15].reshape(3, N, N), np.rot90((N - 1 - b).swapaxes(1, 2), 3, axes=(1, 2)))
    # a group: an image of an image is an image, and the composition runs through all 16 (on a board without symmetry of its own)
    one = [tuple(x) for x in imgs[:, 0]]
    if N >= 5:
        assert len(set(one)) == 16
    for k in range(16):
        again = quench.board_images(N, imgs[k])[:, 0]
        assert {tuple(x) for x in again} == set(one), k
    # the nearest image of an image of A is A, at distance 0; the smallest index on ties
    for k in range(16):
        img, idx, dist = quench.nearest_image(N, s, imgs[k])
        np.testing.assert_array_equal(img, s)
        assert (dist == 0).all() and idx.dtype == np.int32 and dist.dtype == np.int32
        if N >= 5:
            np.testing.assert_array_equal(quench.board_images(N, imgs[k])[idx, np.arange(3)], s)
    flat = np.zeros((1, N * N), dtype=np.uint8)
    img, idx, dist = quench.nearest_image(N, flat, flat)
    assert idx[0] == 0 and dist[0] == 0  # images 0 .. 7 all tie
    far, idx, dist = quench.nearest_image(N, s, qu.random_boards(N, 3, 50 + N))
    brute = (quench.board_images(N, qu.random_boards(N, 3, 50 + N)) != s[None]).sum(axis=2)
    np.testing.assert_array_equal(dist, brute.min(axis=0))
    np.testing.assert_array_equal(idx, brute.argmin(axis=0))
    with pytest.raises(ValueError, match=">= N"):
        quench.board_images(N, np.full((1, N * N), N, dtype=np.uint8))
    with pytest.raises(ValueError, match=">= N"):
        quench.nearest_image(N, np.full((1, N * N), N, dtype=np.uint8), flat)


@pytest.mark.parametrize("align", (True, False))
def test_the_pool_never_rises_and_counts_its_replacements(align):
    N, n, rounds = 6, 24, 3
    s = ru.minima(N, n, 5)
    seeds = abi.seeds_for(9, n)
    e0 = quench.quench_states_host(N, s, max_passes=1, conflicts=False)["energy_in"]
    prev_state, prev_e = s, e0
    replaced_total = 0
    for k in range(1, rounds + 1):  # the pool behind k rounds is the pool behind k - 1 with one more
        r = quench.relink_pool_host(N, s, seeds, k, align=align, partner_seed=3)
        assert r["n_replaced"].shape == (k,) and r["best_energy"].shape == (k,) and r["energy"].dtype == np.int32
        assert (r["energy"] <= prev_e).all()
        changed = (r["state"] != prev_state).any(axis=1)
        assert int(changed.sum()) == int(r["n_replaced"][-1]) and ((r["energy"] < prev_e) == changed).all()
        np.testing.assert_array_equal(quench.quench_states_host(N, r["state"], max_passes=1, conflicts=False)["energy_in"], r["energy"])
        assert int(r["best_energy"][-1]) == int(r["energy"].min())
        replaced_total += int(r["n_replaced"][-1])
        prev_state, prev_e = r["state"], r["energy"]
    assert replaced_total > 0  # the pool is not idle on these minima
    # the partners: round k relinks slot r with slot r - s_k
    shifts = np.random.RandomState(3).randint(1, n, size=1)
    one = quench.relink_pool_host(N, s, seeds, 1, align=False, partner_seed=3)
    direct = quench.relink_host(N, s, np.roll(s, int(shifts[0]), axis=0), seeds, min_dist=max(1, N * N // 8), walk=0)
    better = direct["energy_out"] < direct["energy_in"]
    np.testing.assert_array_equal(one["state"], np.where(better[:, None], direct["state"], s))
