"""CPU-only: basin hopping in host code (mcq_hop_host) against its NumPy restatement (tests/hop_util.py) on every output; n_hops = 0
against the two quenches, at any first_hop; a cut run against the unbroken one; the stream on both sides of word 2^35, where the
second counter word of a block changes, whole and cut; kick = MCQ_MAX_HOP_KICK compared with and without rejections; the properties of
the outputs; kicks that draw a column twice; every refusal; the layout of the mcq_hop block; and that the compared runs contain rejected,
committed and improving hops and, where a kick has three draws or more, a column drawn twice with different heights."""
import ctypes
import functools
import os
import subprocess
import tempfile

import numpy as np
import pytest

import mcq_amd
from tests import heatbath_util as hb
from tests import hop_util as hu
from tests import quench_util as qu

abi = mcq_amd.abi
quench = mcq_amd.quench
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEARCHES = ("single", "pairs")


def _combos(N):
    """(kick, slack) of the comparisons at N: every pair up to N = 4, and beyond a set that holds each kick and each slack, the restatement
    being slow there."""
    if N <= 4:
        return [(k, s) for k in (1, 2, N + 2) for s in (0, 1, 3)]
    if N <= 6:
        return [(1, 0), (2, 1), (N + 2, 3), (N + 2, 0)]
    return [(2, 0), (N + 2, 1), (1, 3)]


# N -> (chains, hops): small enough for the restatement, whose scan visits every pair of columns
SIZES = {2: (3, 40), 3: (3, 30), 4: (2, 20), 5: (2, 20), 6: (1, 20), 8: (1, 20)}


def _boards(N, n, seed):
    s = qu.random_boards(N, n, seed, over=True)  # bytes >= N among them
    if N == 8:
        s[0, ::5] = 200  # clamped bytes for certain
    return s


@functools.lru_cache(maxsize=None)
def _case(N, search, kick, slack):
    """(boards, seeds, the restatement's result) of one comparison; computed once and shared, never changed."""
    n, hops = SIZES[N]
    s = _boards(N, n, 1000 * N + 10 * kick + slack)
    seeds = abi.seeds_for(77 + N + kick, n)
    return s, seeds, hops, hu.hop_many(N, s, seeds, hops, kick=kick, slack=slack, local_search=search)


@pytest.mark.parametrize("search", SEARCHES)
@pytest.mark.parametrize("N", sorted(SIZES))
def test_host_code_equals_the_restatement(N, search):
    for kick, slack in _combos(N):
        s, seeds, hops, want = _case(N, search, kick, slack)
        if N == 8:
            assert int(s.max()) >= N
        got = quench.hop_host(N, s, seeds, hops, kick=kick, slack=slack, local_search=search, hist=True)
        what = f"N={N} {search} kick={kick} slack={slack}"
        hu.assert_equal(got, want, what)
        n = s.shape[0]
        assert set(got) == set(quench.FIELDS_HOP)
        assert got["state"].dtype == np.uint8 and got["best_state"].dtype == np.uint8 and int(got["state"].max()) < N
        assert got["energy_hist"].shape == (n, hops + 1) and got["energy_hist"].dtype == np.int32
        for k, dt in abi.HOP_DTYPES.items():
            assert got[k].dtype == dt and (k == "energy_hist" or got[k].shape == (n,)), k
        if search == "single":
            assert not got["n_pair_moves"].any()
        assert "energy_hist" not in quench.hop_host(N, s, seeds, 2, kick=kick, slack=slack, local_search=search)


@pytest.mark.parametrize("search", SEARCHES)
def test_the_compared_runs_reject_commit_and_improve(search):
    """The condition on the inputs, per local search and per group of sizes (N <= 4, N = 5 .. 8: the kernel's two smallest paddings),
    from the restatement's own traces."""
    cov = hu.Coverage()
    for N in sorted(SIZES):
        for kick, slack in _combos(N):
            cov.add(4 if N <= 4 else 8, _case(N, search, kick, slack)[3])
    for group in (4, 8):
        print(search, group, cov.check(group))


@pytest.mark.parametrize("search", SEARCHES)
def test_no_hops_is_the_quench(search):
    for N, n in ((3, 6), (6, 5), (12, 3), (17, 2)):
        s = qu.random_boards(N, n, 5 + N, over=True)
        got = quench.hop_host(N, s, abi.seeds_for(1, n), 0, local_search=search, hist=True)
        for first_hop, kick in ((3, 2), (hu.mark_first_hop(5), 5), ((1 << 52) - 1, 1024)):  # no hop, no word: first_hop and kick change nothing
            other = quench.hop_host(N, s, abi.seeds_for(2, n), 0, kick=kick, first_hop=first_hop, local_search=search, hist=True)
            hu.assert_equal(other, got, f"N={N} {search}: n_hops=0 at first_hop={first_hop}")
        if search == "pairs":
            q = quench.quench_pairs_host(N, s, max_rounds=0)
            np.testing.assert_array_equal(got["n_pair_moves"], q["n_pair_moves"])
        else:
            q = quench.quench_states_host(N, s, max_passes=0)
            assert not got["n_pair_moves"].any()
        for k in ("state", "energy_in", "energy_out", "n_moves"):
            np.testing.assert_array_equal(got[k], q[k], err_msg=f"N={N} {search}: {k}")
        np.testing.assert_array_equal(got["best_state"], q["state"])
        for k in ("energy_start", "best_energy"):
            np.testing.assert_array_equal(got[k], q["energy_out"], err_msg=k)
        np.testing.assert_array_equal(got["energy_hist"], q["energy_out"][:, None])
        assert not got["best_hop"].any() and not got["n_accepted"].any() and not got["n_improved"].any()


@pytest.mark.parametrize("search", SEARCHES)
def test_a_cut_run_is_the_unbroken_run(search):
    for N, n, kick, slack in ((5, 6, 3, 1), (9, 3, 11, 0), (6, 4, 2, 2)):
        s = qu.random_boards(N, n, 40 + N, over=True)
        seeds = abi.seeds_for(9, n)
        kw = dict(kick=kick, slack=slack, local_search=search, hist=True)
        whole = quench.hop_host(N, s, seeds, 30, first_hop=4, **kw)
        parts, state, done = [], s, 4
        for hops in (7, 1, 22):
            parts.append(quench.hop_host(N, state, seeds, hops, first_hop=done, **kw))
            state, done = parts[-1]["state"], done + hops
        for p in parts[1:]:  # item 3 moves nothing on a fixed point of L
            np.testing.assert_array_equal(p["energy_in"], p["energy_start"])
        merged = hu.merge(parts)
        hu.assert_equal(merged, whole, f"N={N} {search}: 7 + 1 + 22 hops")
        assert (whole["n_improved"] > 0).any() and (whole["best_hop"] > 8).any(), "no chain improved in the later calls"
        # another first_hop is another run
        assert not np.array_equal(quench.hop_host(N, s, seeds, 30, first_hop=5, **kw)["energy_hist"], whole["energy_hist"])


@pytest.mark.parametrize("search", SEARCHES)
def test_the_stream_beyond_word_2_34(search):
    """Hops whose words lie on both sides of word 2^35, where the second counter word of the block (w >> 34) goes from 1 to 2 inside the
    run -- inside a kick, with the odd kick --, against the restatement, whose words are Python integers; then a run cut 7 + 1 + rest
    across the same mark."""
    for N, n, kick, slack, how in ((4, 3, 3, 1, "numpy"), (5, 2, 4, 0, "numpy"), (13, 2, 15, 2, "host"), (13, 2, 4, 0, "host")):
        first, hops = hu.mark_first_hop(kick), 6
        assert hu.crosses_the_mark(kick, first, hops)
        assert kick % 2 == 0 or (1 << 35) % (2 * kick) != 0  # the odd kicks: word 2^35 is no first word of a kick
        s = qu.random_boards(N, n, 70 + N + kick, over=True)
        seeds = abi.seeds_for(11 + kick, n)
        kw = dict(kick=kick, slack=slack, local_search=search, first_hop=first)
        want = hu.hop_many(N, s, seeds, hops, search=how, **kw)
        hu.assert_equal(quench.hop_host(N, s, seeds, hops, hist=True, **kw), want, f"N={N} {search} kick={kick} first_hop={first}")
        assert any(x != "rejected" and x != "same" for tr in want["trace"] for x in tr), "no hop past the mark changed a placement"
    # the restated word past the mark takes the high counter word: it is not the word of a stream that dropped it
    w = (1 << 35) + 6
    assert hu.word(11, w) == hb.philox(((w >> 2) & hb.MASK, 2, 0, 0), (11, 5))[2] != hb.philox(((w >> 2) & hb.MASK, 0, 0, 0), (11, 5))[2]
    for N, n, kick, slack in ((5, 4, 3, 1), (9, 3, 11, 0)):
        first = hu.mark_first_hop(kick, before=7)  # the kick of the single hop in the middle holds word 2^35
        s = qu.random_boards(N, n, 40 + N, over=True)
        seeds = abi.seeds_for(9, n)
        kw = dict(kick=kick, slack=slack, local_search=search, hist=True)
        assert hu.crosses_the_mark(kick, first + 7, 1)
        whole = quench.hop_host(N, s, seeds, 20, first_hop=first, **kw)
        parts, state, done = [], s, first
        for hops in (7, 1, 12):
            parts.append(quench.hop_host(N, state, seeds, hops, first_hop=done, **kw))
            state, done = parts[-1]["state"], done + hops
        hu.assert_equal(hu.merge(parts), whole, f"N={N} {search}: 7 + 1 + 12 hops across word 2^35")


@pytest.mark.parametrize("N,n,hops,searches", hu.MAX_KICK_CASES)
def test_the_largest_kick(N, n, hops, searches):
    """kick = MCQ_MAX_HOP_KICK, more draws than columns at every N: compared, not only accepted.  Without slack some hops are rejected
    (the whole board is restored), with a slack above every energy none is -- by the restatement's traces."""
    assert hu.MAX_KICK == abi.MAX_HOP_KICK > N * N - 1
    rejected = 0
    for search in searches:
        for accept_all in (False, True):
            s, seeds, hops_, slack, want = hu.max_kick_case(N, search, accept_all)
            assert hops_ == hops and want["redrawn"] == n * hops
            n_rej = sum(tr.count("rejected") for tr in want["trace"])
            assert not accept_all or n_rej == 0
            rejected += n_rej
            got = quench.hop_host(N, s, seeds, hops, kick=hu.MAX_KICK, slack=slack, local_search=search, hist=True)
            hu.assert_equal(got, want, f"N={N} {search} kick={hu.MAX_KICK} slack={slack}")
            if accept_all:
                assert (got["n_accepted"] == hops).all()
    assert rejected >= 2, "no hop was rejected without slack"


@pytest.mark.parametrize("search", SEARCHES)
def test_properties_of_the_outputs(search):
    for idx, (N, n, hops, kick, slack) in enumerate(((4, 8, 30, 2, 0), (7, 6, 25, 9, 1), (12, 4, 20, 14, 3), (13, 3, 12, 2, 0), (16, 2, 10, 18, 2),
                                                     (24, 1, 3, 26, 0))):
        s = qu.random_boards(N, n, 600 + idx, over=idx % 2 == 0)
        seeds = abi.seeds_for(30 + idx, n)
        got = quench.hop_host(N, s, seeds, hops, kick=kick, slack=slack, local_search=search, hist=True)
        what = f"N={N} {search}"
        hist = got["energy_hist"].astype(np.int64)
        assert (np.diff(hist, axis=1) <= slack).all(), f"{what}: the history rises by more than slack"
        np.testing.assert_array_equal(got["best_energy"], hist.min(axis=1), err_msg=what)
        np.testing.assert_array_equal(got["best_hop"], hist.argmin(axis=1), err_msg=what)  # the first of the smallest
        np.testing.assert_array_equal(got["energy_start"], hist[:, 0])
        np.testing.assert_array_equal(got["energy_out"], hist[:, -1])
        assert (got["energy_start"] <= got["energy_in"]).all() and (got["n_accepted"] <= hops).all() and (got["n_improved"] <= got["n_accepted"]).all()
        np.testing.assert_array_equal(got["n_improved"], (np.minimum.accumulate(hist, axis=1)[:, 1:] < np.minimum.accumulate(hist, axis=1)[:, :-1]).sum(axis=1))
        for r in range(n):
            assert qu.energy(N, got["state"][r]) == int(got["energy_out"][r]), what
            assert qu.energy(N, got["best_state"][r]) == int(got["best_energy"][r]), what
        # every state_out and best_state is a fixed point of L, by the quench host calls
        for k in ("state", "best_state"):
            single = quench.quench_states_host(N, got[k])
            assert not single["n_moves"].any(), f"{what}: {k} is no single-move minimum"
            if search == "pairs":
                q = quench.quench_pairs_host(N, got[k])
                assert (q["certified"] == 1).all() and not q["n_pair_moves"].any() and not q["n_moves"].any(), f"{what}: a pair move lowers {k}"
        # in place, and only the placements: every per-chain output is optional
        buf = s.copy()
        q = abi.Hop()
        q.N, q.mode, q.n_chains, q.n_hops, q.kick, q.slack, q.local_search = N, abi.MODE_BOARD, n, hops, kick, slack, abi.HOP_LOCAL_SEARCH[search]
        q.seeds, q.state_in, q.state_out = seeds.ctypes.data, buf.ctypes.data, buf.ctypes.data
        mcq_amd._lib.hop_host(q)
        np.testing.assert_array_equal(buf, got["state"], err_msg=f"{what}: in place")


def test_a_kick_may_draw_a_column_twice():
    for N in (2, 3):
        n, kick = 4, 2 * N * N
        s = qu.random_boards(N, n, 3 + N)
        seeds = abi.seeds_for(5, n)
        for search in SEARCHES:
            want = hu.hop_many(N, s, seeds, 12, kick=kick, slack=1, local_search=search)
            assert want["drawn_twice"] == 12 * n  # more draws than columns
            assert 0 < want["redrawn"] <= want["drawn_twice"]
            hu.assert_equal(quench.hop_host(N, s, seeds, 12, kick=kick, slack=1, local_search=search, hist=True), want, f"N={N} kick={kick} {search}")
    # the later draw of a column wins: the draws of one hop by hand
    draws = hu.kick_draws(3, 11, 0, 18)
    assert len({c for c, _ in draws}) < 18 and all(0 <= c < 9 and 0 <= k < 3 for c, k in draws)
    assert hu.word(11, 5) == hb.philox((1, 0, 0, 0), (11, 5))[1]  # word 5 = entry 1 of block 1 under key word 5


def test_refusals_name_the_field():
    L = mcq_amd._lib.lib()
    buf = np.zeros((4, 36), dtype=np.uint8)
    seeds = abi.seeds_for(1, 4)
    hist = np.zeros((4, 8), dtype=np.int32)

    def block(**kw):
        q = abi.Hop()
        q.N, q.mode, q.n_chains, q.n_hops, q.first_hop, q.kick, q.slack, q.local_search = 6, abi.MODE_BOARD, 4, 3, 0, 2, 0, abi.HOP_PAIRS
        q.seeds, q.state_in, q.state_out = seeds.ctypes.data, buf.ctypes.data, buf.ctypes.data
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    refused = ((dict(mode=abi.MODE_FULL3D), b"mode"), (dict(mode=7), b"mode"), (dict(N=1), b"N out of range"), (dict(N=33), b"N out of range"),
               (dict(N=128), b"N out of range"), (dict(n_chains=0), b"n_chains"), (dict(n_chains=-1), b"n_chains"), (dict(n_chains=1 << 31), b"n_chains"),
               (dict(n_hops=-1), b"n_hops"), (dict(first_hop=-1), b"first_hop"), (dict(slack=-1), b"slack"), (dict(kick=0), b"kick out of range"),
               (dict(kick=1025), b"kick out of range"), (dict(kick=-2), b"kick out of range"), (dict(local_search=2), b"local_search"),
               (dict(local_search=-1), b"local_search"), (dict(seeds=None), b"seeds"), (dict(state_in=None), b"state_in"),
               (dict(state_out=None), b"state_out"), (dict(energy_hist=hist.ctypes.data, hist_stride=3), b"hist_stride"),
               (dict(energy_hist=hist.ctypes.data, hist_stride=0), b"hist_stride"),
               (dict(kick=1, n_hops=0, first_hop=1 << 62), b"2^63"), (dict(kick=1024, n_hops=0, first_hop=1 << 52), b"2^63"),
               (dict(kick=2, n_hops=(1 << 63) - 1, first_hop=(1 << 63) - 1), b"2^63"))
    before = L.mcq_quench_pairs_last_error()
    for kw, msg in refused:
        for fn in (L.mcq_hop_host, lambda q: L.mcq_hop_device(q, None)):  # refused before any launch: no GPU here
            assert fn(ctypes.byref(block(**kw))) == abi.EINVAL, kw
            assert msg in L.mcq_hop_last_error(), (kw, L.mcq_hop_last_error())
    assert L.mcq_quench_pairs_last_error() == before  # the message is the call's own
    assert L.mcq_hop_host(None) == abi.EINVAL and L.mcq_hop_device(None, None) == abi.EINVAL
    # at the bounds: accepted (no hop is run: the words are only counted)
    assert L.mcq_hop_host(ctypes.byref(block(kick=1, n_hops=0, first_hop=(1 << 62) - 1))) == abi.OK
    assert L.mcq_hop_host(ctypes.byref(block(energy_hist=hist.ctypes.data, hist_stride=4))) == abi.OK
    assert L.mcq_hop_host(ctypes.byref(block(hist_stride=0))) == abi.OK  # not read without energy_hist
    assert L.mcq_hop_host(ctypes.byref(block(kick=1024))) == abi.OK
    assert abi.MAX_HOP_KICK == 1024 and (abi.HOP_SINGLE, abi.HOP_PAIRS) == (0, 1)
    with pytest.raises(ValueError, match="N out of range"):
        quench.hop_host(33, np.zeros((2, 33 * 33), dtype=np.uint8), seeds[:2], 1)
    with pytest.raises(ValueError, match="kick out of range"):
        quench.hop_host(6, buf, seeds, 1, kick=0)
    with pytest.raises(ValueError, match="slack"):
        quench.hop_host(6, buf, seeds, 1, slack=-1)
    with pytest.raises(ValueError, match="n_chains"):
        quench.hop_host(6, np.zeros((0, 36), dtype=np.uint8), seeds[:0], 1)
    with pytest.raises(ValueError, match="local_search"):
        quench.hop_host(6, buf, seeds, 1, local_search="triples")
    with pytest.raises(ValueError, match="seeds"):
        quench.hop_host(6, buf, seeds[:3], 1)
    with pytest.raises(ValueError, match="final_state layout"):
        quench.hop_host(6, np.zeros((2, 35), dtype=np.uint8), seeds[:2], 1)
    # the competition hook refuses what basin hopping does not run before anything is launched
    for kw, msg in ((dict(N=33, hops=3), "N out of range"), (dict(N=6, hops=-1), "hops must be"), (dict(N=6, hops=3, hop_kick=0), "hop_kick out of range"),
                    (dict(N=6, hops=3, hop_kick=2000), "hop_kick out of range")):
        with pytest.raises(ValueError, match=msg):
            mcq_amd.drivers.run_competition(n_runs=4, n_steps=10, **kw)
    with pytest.raises(ValueError, match="boards only"):
        quench.check_hops(3, 2, 6, board=False)


def test_struct_layout_and_build():
    fields = [f for f, _ in abi.Hop._fields_]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "mcq.h"\nint main(){printf("%zu %d %d %d %d", sizeof(mcq_hop), MCQ_ABI_VERSION, ' \
        'MCQ_MAX_HOP_KICK, MCQ_HOP_SINGLE, MCQ_HOP_PAIRS);' + "".join(f'printf(" %zu", offsetof(mcq_hop, {f}));' for f in fields) + "return 0;}"
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(prog)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")], check=True)
        out = subprocess.run([os.path.join(d, "t")], capture_output=True, text=True, check=True).stdout.split()
    assert int(out[0]) == ctypes.sizeof(abi.Hop) and int(out[1]) == 6 == abi.ABI_VERSION
    assert [int(x) for x in out[2:5]] == [abi.MAX_HOP_KICK, abi.HOP_SINGLE, abi.HOP_PAIRS]
    assert [int(x) for x in out[5:]] == [getattr(abi.Hop, f).offset for f in fields]
    assert set(abi.HOP_DTYPES) | {"state", "best_state"} == set(hu.FIELDS) | {"energy_hist"} == set(quench.FIELDS_HOP)
    b = mcq_amd.build
    assert b.HOP_SOURCES == [os.path.join(b.CSRC, "mcq_hop.hip")] and os.path.exists(b.HOP_SOURCES[0])
    assert not set(b.HOP_SOURCES) & set(b.SOURCES + b.ADDED_SOURCES + b.TEMPER_SOURCES + b.TEMPER3D_SOURCES + b.PAIRS_SOURCES)
    L = mcq_amd._lib.lib()
    for name in ("mcq_hop_device", "mcq_hop_host", "mcq_hop_last_error"):
        assert hasattr(L, name), name
