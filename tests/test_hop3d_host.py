"""CPU-only: basin hopping of full_3d placements in host code (mcq_hop3d_host) against its NumPy restatement (tests/hop3d_util.py) on
every output, with the restatement's own descent at N <= 4 and around the library's quench host call beyond; n_hops = 0 against the
quench, at any first_hop; a cut run against the unbroken one; a repeated placement among sound ones; every refusal through both entry
points; the LDS refusal of the device entry; the layout of the mcq_hop3d block; the build list; the refusal of the annealing hook on
boards; queens_of_boards; and that the compared runs contain rejected, committed and improving hops, draws onto occupied cells and
queens drawn twice."""
import ctypes
import functools
import os
import subprocess
import tempfile

import numpy as np
import pytest

import mcq_amd
from tests import heatbath_util as hb
from tests import hop3d_util as h3
from tests import quench3d_util as q3
from tests import quench_util as qu

abi = mcq_amd.abi
quench = mcq_amd.quench
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (N, Q, chains, hops) with the restatement's own descent: Q = N^2, and the two ends of Q at N = 4
SMALL = ((2, None, 3, 12), (3, None, 3, 12), (4, None, 3, 12), (4, 2, 3, 12), (4, 63, 2, 8))
# (N, chains, hops) around the library's descent: both ends of the kernel's W = 64 | 256 | 1024 ranges meet here
LARGE = ((12, 3, 8), (13, 2, 6), (19, 2, 4), (20, 2, 3))


def _combos(N):
    return [(k, s) for k in (1, 3, N + 2) for s in (0, 2)]


@functools.lru_cache(maxsize=None)
def _small(N, Q, n, hops, kick, slack):
    """(placements, seeds, the restatement's result) of one comparison; computed once and shared, never changed."""
    s = q3.random_placements(N, n, 100 * N + 10 * kick + slack + (Q or 0), Q=Q, over=True)
    seeds = abi.seeds_for(31 + N + kick, n)
    return s, seeds, h3.hop_many(N, s, seeds, hops, Q=Q, kick=kick, slack=slack)


@pytest.mark.parametrize("N,Q,n,hops", SMALL)
def test_host_code_equals_the_restatement(N, Q, n, hops):
    for kick, slack in _combos(N):
        s, seeds, want = _small(N, Q, n, hops, kick, slack)
        got = quench.hop_queens_host(N, s, seeds, hops, Q=Q, kick=kick, slack=slack, hist=True)
        h3.assert_equal(got, want, f"N={N} Q={Q} kick={kick} slack={slack}")
        assert set(got) == set(quench.FIELDS_HOP3D)
        assert got["state"].dtype == np.uint8 and got["best_state"].dtype == np.uint8 and int(got["state"].max()) < N
        assert got["state"].shape == s.shape == got["best_state"].shape
        assert got["energy_hist"].shape == (n, hops + 1) and got["energy_hist"].dtype == np.int32
        for k, dt in abi.HOP3D_DTYPES.items():
            assert got[k].dtype == dt and (k == "energy_hist" or got[k].shape == (n,)), k
        assert "energy_hist" not in quench.hop_queens_host(N, s, seeds, 2, Q=Q, kick=kick, slack=slack)


def test_the_compared_runs_reject_commit_and_improve():
    """The condition on the inputs, from the restatement's own traces, over the comparisons above."""
    cov = h3.Coverage()
    for N, Q, n, hops in SMALL:
        for kick, slack in _combos(N):
            cov.add("small", _small(N, Q, n, hops, kick, slack)[2])
    print(cov.check("small"))


@pytest.mark.parametrize("N,n,hops", LARGE)
def test_host_code_equals_the_loop_around_the_host_descent(N, n, hops):
    changed = 0
    for kick, slack in ((N + 2, 0), (3, 2), (1, 0)):
        s = q3.random_placements(N, n, 7 * N + kick, over=True)
        seeds = abi.seeds_for(5 + N + kick, n)
        want = h3.hop_many(N, s, seeds, hops, kick=kick, slack=slack, search="host")
        got = quench.hop_queens_host(N, s, seeds, hops, kick=kick, slack=slack, hist=True)
        h3.assert_equal(got, want, f"N={N} kick={kick} slack={slack}")
        changed += sum(tr.count("changed") + tr.count("improved") for tr in want["trace"])
    assert changed >= 3


def test_no_hops_is_the_quench():
    for N, Q, n in ((3, None, 5), (4, 40, 4), (7, None, 3), (13, None, 2)):
        s = q3.random_placements(N, n, 5 + N, Q=Q, over=True)
        got = quench.hop_queens_host(N, s, abi.seeds_for(1, n), 0, Q=Q, hist=True)
        for first_hop, kick in ((3, 2), (h3.mark_first_hop(5), 5), ((1 << 52) - 1, 1024)):  # no hop, no word: first_hop and kick change nothing
            other = quench.hop_queens_host(N, s, abi.seeds_for(2, n), 0, Q=Q, kick=kick, first_hop=first_hop, hist=True)
            h3.assert_equal(other, got, f"N={N}: n_hops=0 at first_hop={first_hop}")
        q = quench.quench_queens_host(N, s, Q=Q, max_passes=0)
        for k in ("state", "energy_in", "energy_out", "n_moves", "n_passes", "flags"):
            np.testing.assert_array_equal(got[k], q[k], err_msg=f"N={N}: {k}")
        np.testing.assert_array_equal(got["best_state"], q["state"])
        for k in ("energy_start", "best_energy"):
            np.testing.assert_array_equal(got[k], q["energy_out"], err_msg=k)
        np.testing.assert_array_equal(got["energy_hist"], q["energy_out"][:, None])
        assert not got["best_hop"].any() and not got["n_accepted"].any() and not got["n_improved"].any() and not got["n_kicked"].any()


def test_a_cut_run_is_the_unbroken_run():
    for N, Q, n, kick, slack in ((4, None, 5, 3, 1), (6, 50, 3, 8, 0), (9, None, 3, 11, 2)):
        s = q3.random_placements(N, n, 40 + N, Q=Q, over=True)
        seeds = abi.seeds_for(9, n)
        kw = dict(Q=Q, kick=kick, slack=slack, hist=True)
        whole = quench.hop_queens_host(N, s, seeds, 24, first_hop=4, **kw)
        parts, state, done = [], s, 4
        for hops in (7, 1, 16):
            parts.append(quench.hop_queens_host(N, state, seeds, hops, first_hop=done, **kw))
            state, done = parts[-1]["state"], done + hops
        for p in parts[1:]:  # item 3 moves nothing on a fixed point of L
            np.testing.assert_array_equal(p["energy_in"], p["energy_start"])
        h3.assert_equal(h3.merge(parts), whole, f"N={N}: 7 + 1 + 16 hops")
        assert (whole["n_improved"] > 0).any() and (whole["best_hop"] > 8).any(), "no chain improved in the later calls"
        assert not np.array_equal(quench.hop_queens_host(N, s, seeds, 24, first_hop=5, **kw)["energy_hist"], whole["energy_hist"])


def test_the_stream_beyond_word_2_34():
    """Hops whose words lie on both sides of word 2^35, where the second counter word of the block (w >> 34) goes from 1 to 2 inside the
    run -- inside a kick, with the odd kick --, against the restatement, whose words are Python integers."""
    for N, n, kick, slack, how in ((4, 3, 3, 1, "numpy"), (13, 2, 15, 2, "host")):
        first, hops = h3.mark_first_hop(kick), 6
        assert h3.crosses_the_mark(kick, first, hops) and (1 << 35) % (2 * kick) != 0
        s = q3.random_placements(N, n, 70 + N + kick, over=True)
        seeds = abi.seeds_for(11 + kick, n)
        kw = dict(kick=kick, slack=slack, first_hop=first)
        want = h3.hop_many(N, s, seeds, hops, search=how, **kw)
        h3.assert_equal(quench.hop_queens_host(N, s, seeds, hops, hist=True, **kw), want, f"N={N} kick={kick} first_hop={first}")
        assert any(x in ("changed", "improved") for tr in want["trace"] for x in tr), "no hop past the mark changed a placement"
    w = (1 << 35) + 6
    assert h3.word(11, w) == hb.philox(((w >> 2) & hb.MASK, 2, 0, 0), (11, 6))[2] != hb.philox(((w >> 2) & hb.MASK, 0, 0, 0), (11, 6))[2]
    assert h3.word(11, 5) == hb.philox((1, 0, 0, 0), (11, 6))[1] != hb.philox((1, 0, 0, 0), (11, 5))[1]  # key word 6, not mcq_hop's 5


def test_a_repeated_placement_is_flagged_and_unmoved():
    for N, Q in ((4, None), (13, None), (5, 30)):
        Qn = N * N if Q is None else Q
        n, hops = 5, 4
        s = q3.random_placements(N, n, 20 + N, Q=Q, over=True)
        sound = s.copy()
        s[1, 3:6] = s[1, 0:3]  # queen 1 onto queen 0
        s[3, -3:] = np.minimum(s[3, 0:3], N - 1)
        s[3, 0:3] = np.where(s[3, 0:3] == N - 1, 250, s[3, 0:3])  # the same cell once the bytes are clamped
        seeds = abi.seeds_for(8, n)
        got = quench.hop_queens_host(N, s, seeds, hops, Q=Q, kick=3, hist=True)
        ref = quench.hop_queens_host(N, sound, seeds, hops, Q=Q, kick=3, hist=True)
        np.testing.assert_array_equal(got["flags"], [0, abi.HOP3D_REPEATED, 0, abi.HOP3D_REPEATED, 0])
        for r in (1, 3):
            e = q3.pairwise_energy(N, s[r])
            np.testing.assert_array_equal(got["state"][r], np.minimum(s[r], N - 1))
            np.testing.assert_array_equal(got["best_state"][r], np.minimum(s[r], N - 1))
            for k in ("energy_in", "energy_start", "energy_out", "best_energy"):
                assert int(got[k][r]) == e, k
            for k in ("best_hop", "n_accepted", "n_improved", "n_moves", "n_passes", "n_kicked"):
                assert int(got[k][r]) == 0, k
            assert (got["energy_hist"][r] == e).all() and got["energy_hist"].shape[1] == hops + 1
        for r in (0, 2, 4):  # the neighbours are those of the call without a repeat
            for k in quench.FIELDS_HOP3D:
                np.testing.assert_array_equal(got[k][r], ref[k][r], err_msg=f"N={N} chain {r}: {k}")
        want = h3.hop_many(N, s, seeds, hops, Q=Qn, kick=3, search="host")
        h3.assert_equal(got, want, f"N={N}: a repeat among sound placements")


def test_properties_of_the_outputs():
    for idx, (N, Q, n, hops, kick, slack) in enumerate(((4, None, 6, 30, 2, 0), (7, 30, 4, 20, 9, 1), (12, None, 3, 12, 14, 3), (13, None, 2, 8, 2, 0))):
        s = q3.random_placements(N, n, 600 + idx, Q=Q, over=idx % 2 == 0)
        seeds = abi.seeds_for(30 + idx, n)
        got = quench.hop_queens_host(N, s, seeds, hops, Q=Q, kick=kick, slack=slack, hist=True)
        hist = got["energy_hist"].astype(np.int64)
        assert (np.diff(hist, axis=1) <= slack).all(), f"N={N}: the history rises by more than slack"
        np.testing.assert_array_equal(got["best_energy"], hist.min(axis=1))
        np.testing.assert_array_equal(got["best_hop"], hist.argmin(axis=1))  # the first of the smallest
        np.testing.assert_array_equal(got["energy_start"], hist[:, 0])
        np.testing.assert_array_equal(got["energy_out"], hist[:, -1])
        assert (got["energy_start"] <= got["energy_in"]).all() and (got["n_accepted"] <= hops).all() and (got["n_improved"] <= got["n_accepted"]).all()
        assert (got["n_kicked"] <= hops * kick).all() and (got["n_passes"] >= hops + 1).all()
        for r in range(n):
            assert q3.pairwise_energy(N, got["state"][r]) == int(got["energy_out"][r])
            assert q3.pairwise_energy(N, got["best_state"][r]) == int(got["best_energy"][r])
            assert not q3.is_repeated(N, got["state"][r]) and not q3.is_repeated(N, got["best_state"][r])
        for k in ("state", "best_state"):  # every state_out and best_state is a fixed point of L
            q = quench.quench_queens_host(N, got[k], Q=Q)
            assert not q["n_moves"].any() and (q["n_passes"] == 1).all(), f"N={N}: {k} is no minimum"
        # in place, and only the placements: every per-chain output is optional
        buf = s.copy()
        q = abi.Hop3d()
        q.N, q.n_queens, q.n_chains, q.n_hops, q.kick, q.slack = N, Q or 0, n, hops, kick, slack
        q.seeds, q.state_in, q.state_out = seeds.ctypes.data, buf.ctypes.data, buf.ctypes.data
        mcq_amd._lib.hop3d_host(q)
        np.testing.assert_array_equal(buf, got["state"], err_msg=f"N={N}: in place")


def test_the_quick_certificate_is_the_slow_one():
    """hop3d_util.is_local_minimum, which the GPU tests take at N = 13 and 20, against quench3d_util.is_local_minimum: on outputs of the
    hops (minima), on the same with one queen moved to a free cell, and on random placements."""
    seen = set()
    for N, Q, n in ((3, None, 4), (5, 30, 3), (6, None, 3), (8, None, 2)):
        s = q3.random_placements(N, n, 50 + N, Q=Q)
        out = quench.hop_queens_host(N, s, abi.seeds_for(3, n), 4, Q=Q, kick=3)["state"]
        rs = np.random.RandomState(N)
        for r in range(n):
            moved = out[r].copy().reshape(-1, 3)
            while True:
                cell = rs.randint(0, N, size=3)
                if not (moved == cell).all(axis=1).any():
                    break
            moved[rs.randint(len(moved))] = cell
            for z in (out[r], moved.reshape(-1), s[r]):
                slow = q3.is_local_minimum(N, z)
                assert h3.is_local_minimum(N, z) == slow
                seen.add(slow)
            assert q3.is_local_minimum(N, out[r])
    assert seen == {True, False}


def test_refusals_name_the_field():
    L = mcq_amd._lib.lib()
    buf = np.zeros((4, 108), dtype=np.uint8)
    seeds = abi.seeds_for(1, 4)
    hist = np.zeros((4, 8), dtype=np.int32)

    def block(**kw):
        q = abi.Hop3d()
        q.N, q.n_queens, q.n_chains, q.n_hops, q.first_hop, q.kick, q.slack = 6, 0, 4, 3, 0, 2, 0
        q.seeds, q.state_in, q.state_out = seeds.ctypes.data, buf.ctypes.data, buf.ctypes.data
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    refused = ((dict(N=1), b"N out of range"), (dict(N=33), b"the full_3d hop stops at N = 32"), (dict(N=64), b"the full_3d hop stops at N = 32"),
               (dict(N=65), b"N out of range"), (dict(N=-3), b"N out of range"), (dict(n_queens=1), b"n_queens out of range"),
               (dict(n_queens=216), b"n_queens out of range"), (dict(n_queens=-1), b"n_queens out of range"),
               (dict(n_chains=0), b"n_chains"), (dict(n_chains=-1), b"n_chains"), (dict(n_chains=1 << 31), b"n_chains"),
               (dict(n_hops=-1), b"n_hops"), (dict(first_hop=-1), b"first_hop"), (dict(slack=-1), b"slack"), (dict(kick=0), b"kick out of range"),
               (dict(kick=1025), b"kick out of range"), (dict(kick=-2), b"kick out of range"), (dict(seeds=None), b"seeds"),
               (dict(state_in=None), b"state_in"), (dict(state_out=None), b"state_out"),
               (dict(energy_hist=hist.ctypes.data, hist_stride=3), b"hist_stride"), (dict(energy_hist=hist.ctypes.data, hist_stride=0), b"hist_stride"),
               (dict(kick=1, n_hops=0, first_hop=1 << 62), b"2^63"), (dict(kick=1024, n_hops=0, first_hop=1 << 52), b"2^63"),
               (dict(kick=2, n_hops=(1 << 63) - 1, first_hop=(1 << 63) - 1), b"2^63"))
    before = L.mcq_hop_last_error(), L.mcq_quench3d_last_error()
    for kw, msg in refused:
        for fn in (L.mcq_hop3d_host, lambda q: L.mcq_hop3d_device(q, None)):  # refused before any launch: no GPU here
            assert fn(ctypes.byref(block(**kw))) == abi.EINVAL, kw
            assert msg in L.mcq_hop3d_last_error(), (kw, L.mcq_hop3d_last_error())
    assert (L.mcq_hop_last_error(), L.mcq_quench3d_last_error()) == before  # the message is the call's own
    assert L.mcq_hop3d_host(None) == abi.EINVAL and L.mcq_hop3d_device(None, None) == abi.EINVAL
    assert b"NULL parameter block" in L.mcq_hop3d_last_error()
    # at the bounds: accepted (no hop is run: the words are only counted)
    assert L.mcq_hop3d_host(ctypes.byref(block(kick=1, n_hops=0, first_hop=(1 << 62) - 1))) == abi.OK
    assert L.mcq_hop3d_host(ctypes.byref(block(energy_hist=hist.ctypes.data, hist_stride=4))) == abi.OK
    assert L.mcq_hop3d_host(ctypes.byref(block(hist_stride=0))) == abi.OK  # not read without energy_hist
    assert L.mcq_hop3d_host(ctypes.byref(block(kick=1024, n_queens=2))) == abi.OK
    assert L.mcq_hop3d_host(ctypes.byref(block(N=3, n_queens=26))) == abi.OK
    with pytest.raises(ValueError, match="N out of range"):
        quench.hop_queens_host(33, np.zeros((2, 3 * 33 * 33), dtype=np.uint8), seeds[:2], 1)
    with pytest.raises(ValueError, match="kick out of range"):
        quench.hop_queens_host(6, buf, seeds, 1, kick=0)
    with pytest.raises(ValueError, match="slack"):
        quench.hop_queens_host(6, buf, seeds, 1, slack=-1)
    with pytest.raises(ValueError, match="n_chains"):
        quench.hop_queens_host(6, np.zeros((0, 108), dtype=np.uint8), seeds[:0], 1)
    with pytest.raises(ValueError, match="seeds"):
        quench.hop_queens_host(6, buf, seeds[:3], 1)
    with pytest.raises(ValueError, match="final_state layout of full_3d"):
        quench.hop_queens_host(6, np.zeros((2, 107), dtype=np.uint8), seeds[:2], 1)


def test_the_device_entry_refuses_what_the_lds_does_not_hold():
    """N = 32: Q = 23 520 is the largest chain of 160 KiB, and Q = 23 521 is refused by the device entry before any launch -- no GPU is
    touched here -- and taken by the host entry.  (The host call is handed a repeated placement, all queens in two cells: it is
    recounted and not descended, which at this shape takes half a minute.)"""
    L = mcq_amd._lib.lib()
    assert abi.MAX_HOP3D_LDS == 160 * 1024
    assert abi.hop3d_lds_bytes(32, 23520) == abi.MAX_HOP3D_LDS < abi.hop3d_lds_bytes(32, 23521)
    assert abi.hop3d_lds_bytes(32, 23519) == abi.MAX_HOP3D_LDS  # (two queens to a dword)
    for N in range(2, 33):  # every Q = N^2 fits; the bytes are the quench's and one more copy of the queens
        cells, cpd = N ** 3, 4 if N <= 19 else 2
        assert abi.hop3d_lds_bytes(N) == abi.hop3d_lds_bytes(N, 0) == 4 * (32 + -(-cells // cpd) + -(-cells // 32) + 2 * -(-N * N // 2)) <= abi.MAX_HOP3D_LDS
    assert abi.hop3d_lds_bytes(19, 19 ** 3 - 1) <= abi.MAX_HOP3D_LDS  # below N = 20 every Q fits
    Q, n = 23521, 1
    s = np.zeros((n, Q, 3), dtype=np.uint8)
    s[:, 1::2] = 31
    s = s.reshape(n, 3 * Q)
    seeds = abi.seeds_for(1, n)
    out = np.zeros_like(s)
    q = abi.Hop3d()
    q.N, q.n_queens, q.n_chains, q.n_hops, q.kick = 32, Q, n, 0, 2
    q.seeds, q.state_in, q.state_out = seeds.ctypes.data, s.ctypes.data, out.ctypes.data
    assert L.mcq_hop3d_device(ctypes.byref(q), None) == abi.EINVAL
    msg = L.mcq_hop3d_last_error().decode()
    assert "N = 32" in msg and "n_queens = 23521" in msg and str(abi.hop3d_lds_bytes(32, Q)) in msg and str(abi.MAX_HOP3D_LDS) in msg, msg
    got = quench.hop_queens_host(32, s, seeds, 0, Q=Q)
    half = (Q + 1) // 2
    pairs = half * (half - 1) // 2 + (Q - half) * (Q - half - 1) // 2 + half * (Q - half)  # the two cells lie on one diagonal
    assert int(got["flags"][0]) == abi.HOP3D_REPEATED and int(got["energy_in"][0]) == int(got["energy_out"][0]) == pairs
    np.testing.assert_array_equal(got["state"], s)
    q.n_queens = 23520  # what fits passes the checks: the next refusal is not the LDS
    q.seeds = None
    assert L.mcq_hop3d_device(ctypes.byref(q), None) == abi.EINVAL and b"seeds" in L.mcq_hop3d_last_error()


def test_struct_layout_and_build():
    fields = [f for f, _ in abi.Hop3d._fields_]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "mcq.h"\nint main(){printf("%zu %d %d %d %d %d", sizeof(mcq_hop3d), MCQ_ABI_VERSION, ' \
        'MCQ_MAX_HOP_KICK, MCQ_MAX_HOP3D_LDS, MCQ_HOP3D_REPEATED, MCQ_MAX_N_QUENCH3D);' + \
        "".join(f'printf(" %zu", offsetof(mcq_hop3d, {f}));' for f in fields) + "return 0;}"
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(prog)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")], check=True)
        out = subprocess.run([os.path.join(d, "t")], capture_output=True, text=True, check=True).stdout.split()
    assert int(out[0]) == ctypes.sizeof(abi.Hop3d) and int(out[1]) == 6 == abi.ABI_VERSION
    assert [int(x) for x in out[2:6]] == [abi.MAX_HOP_KICK, abi.MAX_HOP3D_LDS, abi.HOP3D_REPEATED, abi.MAX_N_QUENCH3D]
    assert [int(x) for x in out[6:]] == [getattr(abi.Hop3d, f).offset for f in fields]
    assert set(abi.HOP3D_DTYPES) | {"state", "best_state"} == set(h3.FIELDS) | {"energy_hist"} == set(quench.FIELDS_HOP3D)
    b = mcq_amd.build
    assert b.HOP3D_SOURCES == [os.path.join(b.CSRC, "mcq_hop3d.hip")] and os.path.exists(b.HOP3D_SOURCES[0])
    assert not set(b.HOP3D_SOURCES) & set(b.SOURCES + b.ADDED_SOURCES + b.TEMPER_SOURCES + b.TEMPER3D_SOURCES + b.PAIRS_SOURCES + b.HOP_SOURCES)
    L = mcq_amd._lib.lib()
    for name in ("mcq_hop3d_device", "mcq_hop3d_host", "mcq_hop3d_last_error"):
        assert hasattr(L, name), name


def test_the_annealing_hook_refuses_boards():
    sp = {"type": "linear_annealing", "beta_start": 1.0, "beta_end": 3.0}
    with pytest.raises(ValueError, match=r"run_competition\(hops="):
        mcq_amd.heatbath.anneal_heatbath(6, 4, "random", sp, abi.seeds_for(1, 16), hops=3)
    with pytest.raises(ValueError, match="hops must be >= 0"):
        mcq_amd.heatbath.anneal_heatbath(6, 4, "random", sp, abi.seeds_for(1, 16), mcmc_type="full_3d", hops=-1)
    for kick in (0, 1025):
        with pytest.raises(ValueError, match="hop_kick out of range"):
            mcq_amd.heatbath.anneal_heatbath(6, 4, "random", sp, abi.seeds_for(1, 16), mcmc_type="full_3d", hops=3, hop_kick=kick)


def test_queens_of_boards_keeps_the_energy():
    for N, n in ((2, 3), (5, 4), (8, 3), (12, 2)):
        boards = qu.random_boards(N, n, 3 + N, over=True)
        z = quench.queens_of_boards(N, boards)
        assert z.shape == (n, 3 * N * N) and z.dtype == np.uint8
        for r in range(n):
            t = z[r].reshape(N, N, 3)
            assert (t[:, :, 0] == np.arange(N)[:, None]).all() and (t[:, :, 1] == np.arange(N)[None, :]).all()
            np.testing.assert_array_equal(t[:, :, 2].reshape(-1), qu.clamp(N, boards[r]))
            assert q3.pairwise_energy(N, z[r]) == qu.energy(N, boards[r]) and not q3.is_repeated(N, z[r])
        got = quench.hop_queens_host(N, z, abi.seeds_for(2, n), 0)
        np.testing.assert_array_equal(got["energy_in"], quench.quench_states_host(N, boards)["energy_in"])
        np.testing.assert_array_equal(quench.queens_of_boards(N, boards[0]), z[:1])  # one board is one chain
