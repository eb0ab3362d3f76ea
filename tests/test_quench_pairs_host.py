"""CPU-only: the pair-move quench in host code (mcq_quench_pairs_host) against its NumPy restatement (tests/quench_pairs_util.py) on every
output, the restatement's scan variants against each other, the properties of the output, max_rounds, in place, every refusal, the
layout of the mcq_quench_pairs block, and that the test sets exercise pair moves at all.

Held independently of the library: host code = restatement to convergence at N = 2, 4, 5, 8, 9, 12, 13, 16 (random boards) and at
N = 17, 24, 25, 32 (minima with columns redrawn; random boards for two rounds), the restatement scanning every aligned pair and every
(k1, k2) without pruning, on inputs whose traces hold every class of pair move (D, delta1, delta2), every line of the board and the
edges of the kernel's table rows and lane loops; and "certified = 1 means no single move and no pair move lowers E" on every output of
test_properties_of_the_output up to N = 32.  Not held: runs to convergence from RANDOM boards beyond N = 16 (a minute each in NumPy);
recounted energies in the scan beyond N = 5 (the formula is pinned to the recount entry for entry up to N = 6)."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

import mcq_amd
from tests import quench_pairs_util as qp
from tests import quench_util as qu

abi = mcq_amd.abi
quench = mcq_amd.quench
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (N, boards): small enough for the restatement, whose scan visits every pair of columns
SIZES = ((2, 6), (3, 8), (4, 8), (5, 6), (6, 4), (8, 2))


def _boards(N, n, seed):
    s = qu.random_boards(N, n, seed, over=True)  # bytes >= N among them
    s[0] = seed % N  # all heights equal
    s[1] = 255       # every byte clamped
    return s


@pytest.mark.parametrize("N,n", SIZES)
def test_host_code_equals_the_restatement(N, n):
    s = _boards(N, n, 300 + N)
    assert int(s.max()) >= N
    want = qp.quench_pairs_many(N, s)
    got = quench.quench_pairs_host(N, s)
    qp.assert_equal(got, want, f"N={N} ({n} boards)")
    assert got["state"].dtype == np.uint8 and got["conflicts"].dtype == np.uint16 and int(got["state"].max()) < N
    for k in qp.FIELDS[1:-1]:
        assert got[k].dtype == np.int32 and got[k].shape == (n,), k
    assert (got["certified"] == 1).all() and (got["n_rounds"] == got["n_pair_moves"] + 1).all()
    assert (got["conflicts"].sum(axis=1) == 2 * got["energy_out"]).all()
    for r in range(n):
        assert len(want["deltas"][r]) == int(got["n_pair_moves"][r]) and all(D in (-1, -2) for D in want["deltas"][r])
        assert int(got["energy_out"][r]) <= int(got["energy_single"][r]) + sum(want["deltas"][r])  # the descents in between lower it further
        assert qu.energy(N, got["state"][r]) == int(got["energy_out"][r])


def _covered(NP):
    """The coverage of group NP from the restatement's traces alone, asserted; every class is required of every group (12 random boards
    at N = 4 do hold a (-1, 0, 0), so no group excepts one)."""
    cov = qp.Coverage()
    for N in qp.GROUPS[NP]:
        cov.add(N, qp.restated_case(N)[1])
    return cov.check(NP, qp.GROUPS[NP][1])


@pytest.mark.parametrize("NP", sorted(qp.GROUPS))
def test_host_code_equals_the_restatement_at_every_instantiation(NP):
    """Both ends of every padded edge of the kernel, to convergence, against the restatement with the exhaustive vectorised scan: random
    boards up to N = 16, minima with a few columns redrawn beyond (and random boards for two rounds there).  The inputs must hold every
    class of pair move, every line of the board, the last heights of a table row, neighbouring columns, runs of several rounds and,
    beyond N = 16, a second column past the 64th slot -- by the restatement's traces, before the comparison counts."""
    print(NP, _covered(NP))
    for N in qp.GROUPS[NP]:
        s, want = qp.restated_case(N)
        assert int(s.max()) >= N
        got = quench.quench_pairs_host(N, s)
        qp.assert_equal(got, want, f"N={N} ({s.shape[0]} boards)")
        assert (got["certified"] == 1).all()
        for r in range(s.shape[0] if N <= 16 else 1):
            qp.certify(N, got["state"][r], f"N={N} board {r}")
            assert qu.energy(N, got["state"][r]) == int(got["energy_out"][r])
        if N > 16:  # from random boards, where the first descent is long and the first scans see many candidates
            s = qu.random_boards(N, 1, 300 + N, over=True)
            want = qp.quench_pairs_many(N, s, 2, pairs="fast")
            assert int(want["certified"][0]) == 0 and len(want["trace"][0]) == 2
            qp.assert_equal(quench.quench_pairs_host(N, s, max_rounds=2), want, f"N={N}, a random board, max_rounds=2")


def test_fast_scan_equals_the_slow_scans():
    """The vectorised scan against the scan over ALL pairs with recounted energies on single-move minima at N = 2 .. 5, and against the
    scan over all pairs by the formula at N = 6 .. 8, on the minimum and on what the first pair moves lead to."""
    checked = improving = 0
    for N, n, slow in ((2, 6, "recount"), (3, 10, "recount"), (4, 10, "recount"), (5, 6, "recount"), (6, 4, "formula"), (7, 3, "formula"), (8, 2, "formula")):
        for s in qu.random_boards(N, n, 140 + N):
            h = qu.quench(N, s)["state"].astype(np.int64)
            for _ in range(3):
                assert qu.is_local_minimum(N, h)
                every = qp.scan(N, h, "all", slow)
                assert qp.fast_scan(N, h) == every, (N, h)
                checked += 1
                if every[0] >= 0:
                    break
                improving += 1
                h[every[1]], h[every[2]] = every[3], every[4]
                h = qu.quench(N, h)["state"].astype(np.int64)
    assert checked >= 60 and improving >= 20
    # off a single-move minimum the scans differ only by pairs that are not aligned: over the aligned pairs they agree on any board
    for N in (3, 5):
        h = qu.clamp(N, qu.random_boards(N, 1, 90 + N)[0])
        assert qp.fast_scan(N, h) == qp.scan(N, h, "aligned", "formula")
    # the restated runs themselves, slow scan against fast
    for N, n in ((4, 6), (6, 3)):
        s = qu.random_boards(N, n, 77 + N, over=True)
        slow, fast = qp.quench_pairs_many(N, s), qp.quench_pairs_many(N, s, pairs="fast")
        qp.assert_equal(fast, slow, f"N={N}: restated runs")
        assert fast["deltas"] == slow["deltas"] == [[m["D"] for m in tr] for tr in fast["trace"]]
    assert qp.lane_slot(17, 0, 16 * 17 + 16) == 2 * 17 + 16 and qp.family(17, 16, 16 * 17) == "antidiagonal" and qp.lane_slot(5, 7, 17) == 5 + 3


def test_klarner_board_comes_back_untouched_and_certified():
    h = qu.klarner(11)
    assert qu.energy(11, h) == 0
    got = quench.quench_pairs_host(11, h)
    np.testing.assert_array_equal(got["state"][0], h)
    for k, v in (("energy_in", 0), ("energy_single", 0), ("energy_out", 0), ("n_moves", 0), ("n_pair_moves", 0), ("n_rounds", 1), ("certified", 1)):
        assert int(got[k][0]) == v, k
    assert not got["conflicts"].any()


def test_scan_variants_agree():
    """On single-move minima the scan over all pairs equals the scan over aligned pairs (N <= 5), and the formula equals the recount."""
    checked = 0
    for N, n in ((3, 10), (4, 10), (5, 6)):
        for s in qu.random_boards(N, n, 40 + N):
            h = qu.quench(N, s)["state"].astype(np.int64)
            for _ in range(3):  # the minimum, and what the first pair moves lead to
                every = qp.scan(N, h, "all", "recount")
                assert every == qp.scan(N, h, "aligned", "recount") == qp.scan(N, h, "all", "formula") == qp.scan(N, h, "aligned", "formula"), (N, h)
                checked += 1
                if every[0] >= 0:
                    break
                h[every[1]], h[every[2]] = every[3], every[4]
                h = qu.quench(N, h)["state"].astype(np.int64)
    assert checked >= 40
    # the formula against the recount entry for entry, on boards that are no minima of anything
    for N in (2, 3, 4, 5, 6):
        h = qu.clamp(N, qu.random_boards(N, 1, 90 + N)[0])
        aligned, _ = qp.geometry(N)
        t = qu.table(N, h)
        for c1 in range(N * N):
            for c2 in range(c1 + 1, N * N):
                f, r = qp.pair_deltas(N, h, c1, c2, "formula", t), qp.pair_deltas(N, h, c1, c2, "recount")
                keep = np.ones((N, N), dtype=bool)
                keep[h[c1], :] = keep[:, h[c2]] = False
                np.testing.assert_array_equal(f[keep], r[keep], err_msg=f"N={N} pair ({c1}, {c2})")
                # a pair that is not aligned: the sum of the two single-move differences
                assert aligned[c1, c2] or (f == (t[c1] - t[c1][h[c1]])[:, None] + (t[c2] - t[c2][h[c2]])[None, :]).all()


def test_properties_of_the_output():
    for idx, N in enumerate((2, 3, 4, 5, 7, 9, 12, 13, 16, 17, 24, 32)):
        n = 6 if N <= 9 else 3 if N <= 17 else 1
        s = qu.random_boards(N, n, 8000 + idx, over=idx % 2 == 1)
        got = quench.quench_pairs_host(N, s)
        single = quench.quench_states_host(N, s)
        np.testing.assert_array_equal(got["energy_single"], single["energy_out"], err_msg=f"N={N}: energy_single")
        np.testing.assert_array_equal(got["energy_in"], single["energy_in"])
        # the state behind energy_single is quench_states_host's: fed in, it gives the same run without the first descent's moves
        behind = quench.quench_pairs_host(N, single["state"])
        for k in qp.FIELDS:
            if k == "n_moves":
                np.testing.assert_array_equal(behind[k] + single["n_moves"], got[k], err_msg=f"N={N}: {k}")
            elif k == "energy_in":
                np.testing.assert_array_equal(behind[k], single["energy_out"])
            else:
                np.testing.assert_array_equal(behind[k], got[k], err_msg=f"N={N}: {k} behind the single-move quench")
        assert (got["certified"] == 1).all()
        assert (got["energy_out"] <= got["energy_single"]).all() and (got["energy_single"] <= got["energy_in"]).all()
        assert (got["n_rounds"] == got["n_pair_moves"] + 1).all() and (got["n_rounds"] <= got["energy_in"] + 1).all()
        assert (got["energy_single"] - got["energy_out"] >= got["n_pair_moves"]).all()  # every pair move lowers E by at least 1
        assert ((got["n_pair_moves"] == 0) == (got["energy_out"] == got["energy_single"])).all()
        for r in range(n):
            what = f"N={N} board {r}"
            assert qu.is_local_minimum(N, got["state"][r]), f"{what}: a certified output is no single-move minimum"
            assert qu.energy(N, got["state"][r]) == int(got["energy_out"][r]), what
            qp.certify(N, got["state"][r], what)  # at every N: no candidate of the rule lowers a certified output
            if N <= 4:
                assert not qp.has_improving_pair_by_recount(N, got["state"][r]), f"{what}: a pair move lowers a certified output"
        again = quench.quench_pairs_host(N, got["state"])
        np.testing.assert_array_equal(again["state"], got["state"])
        assert (again["n_moves"] == 0).all() and (again["n_pair_moves"] == 0).all() and (again["n_rounds"] == 1).all() and (again["certified"] == 1).all()
        np.testing.assert_array_equal(again["conflicts"], got["conflicts"])


@pytest.mark.parametrize("max_rounds", (1, 2))
def test_max_rounds(max_rounds):
    cut = 0
    for N, n, seed in ((4, 12, 2), (5, 8, 3), (6, 5, 4)):
        s = qu.random_boards(N, n, seed)
        full = quench.quench_pairs_host(N, s)
        got = quench.quench_pairs_host(N, s, max_rounds=max_rounds)
        qp.assert_equal(got, qp.quench_pairs_many(N, s, max_rounds), f"N={N} max_rounds={max_rounds}")
        assert (got["n_rounds"] <= max_rounds).all() and (got["n_rounds"] == np.minimum(full["n_rounds"], max_rounds)).all()
        # certified exactly where the last scan found nothing: the runs that needed no more than max_rounds scans
        np.testing.assert_array_equal(got["certified"], (full["n_rounds"] <= max_rounds).astype(np.int32))
        np.testing.assert_array_equal(got["n_pair_moves"], np.where(got["certified"] == 1, got["n_rounds"] - 1, got["n_rounds"]))
        for r in range(n):
            assert qu.is_local_minimum(N, got["state"][r]), f"N={N} board {r}: the final descent is missing"
            assert qu.energy(N, got["state"][r]) == int(got["energy_out"][r])
            if got["certified"][r]:
                np.testing.assert_array_equal(got["state"][r], full["state"][r])
        # the rest of the run, from where the limit stopped it
        rest = quench.quench_pairs_host(N, got["state"])
        np.testing.assert_array_equal(rest["state"], full["state"], err_msg=f"N={N}: {max_rounds} rounds, then the rest")
        np.testing.assert_array_equal(got["n_pair_moves"] + rest["n_pair_moves"], full["n_pair_moves"])
        cut += int((got["certified"] == 0).sum())
    assert cut >= 6  # the limit did end runs


def test_in_place_and_optional_outputs():
    for N, n in ((5, 7), (12, 3)):
        s = _boards(N, n, 50 + N)
        want = quench.quench_pairs_host(N, s)
        buf = s.copy()
        q = abi.QuenchPairs()
        q.N, q.mode, q.n_chains, q.max_rounds = N, abi.MODE_BOARD, n, 0
        q.state_in = q.state_out = buf.ctypes.data
        e_out = np.zeros(n, dtype=np.int32)
        q.energy_out = e_out.ctypes.data  # the other outputs are optional
        mcq_amd._lib.quench_pairs_host(q)
        np.testing.assert_array_equal(buf, want["state"], err_msg=f"N={N}: in place")
        np.testing.assert_array_equal(e_out, want["energy_out"])
        assert "conflicts" not in quench.quench_pairs_host(N, s, conflicts=False)


def test_refusals_name_the_field():
    L = mcq_amd._lib.lib()
    buf = np.zeros((4, 36), dtype=np.uint8)

    def block(**kw):
        q = abi.QuenchPairs()
        q.N, q.mode, q.n_chains, q.max_rounds = 6, abi.MODE_BOARD, 4, 0
        q.state_in = q.state_out = buf.ctypes.data
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    refused = ((dict(mode=abi.MODE_FULL3D), b"mode"), (dict(mode=7), b"mode"), (dict(N=1), b"N out of range"), (dict(N=33), b"N out of range"),
               (dict(N=128), b"N out of range"), (dict(N=-3), b"N out of range"), (dict(n_chains=0), b"n_chains"), (dict(n_chains=-1), b"n_chains"),
               (dict(n_chains=1 << 31), b"n_chains"), (dict(max_rounds=-1), b"max_rounds"), (dict(state_in=None), b"state_in"),
               (dict(state_out=None), b"state_out"))
    before = L.mcq_quench_last_error()
    for kw, msg in refused:
        for fn in (L.mcq_quench_pairs_host, lambda q: L.mcq_quench_pairs_device(q, None)):  # refused before any launch: no GPU here
            assert fn(ctypes.byref(block(**kw))) == abi.EINVAL, kw
            assert msg in L.mcq_quench_pairs_last_error(), (kw, L.mcq_quench_pairs_last_error())
    assert L.mcq_quench_last_error() == before  # the message is the call's own
    assert L.mcq_quench_pairs_host(None) == abi.EINVAL and L.mcq_quench_pairs_device(None, None) == abi.EINVAL
    assert L.mcq_quench_pairs_host(ctypes.byref(block())) == abi.OK
    assert abi.MAX_N_QUENCH_PAIRS == 32
    with pytest.raises(ValueError, match="N out of range"):
        quench.quench_pairs_host(33, np.zeros((2, 33 * 33), dtype=np.uint8))
    with pytest.raises(ValueError, match="max_rounds"):
        quench.quench_pairs_host(6, buf, max_rounds=-2)
    with pytest.raises(ValueError, match="n_chains"):
        quench.quench_pairs_host(6, np.zeros((0, 36), dtype=np.uint8))
    with pytest.raises(ValueError, match="final_state layout"):
        quench.quench_pairs_host(6, np.zeros((2, 35), dtype=np.uint8))
    assert quench.quench_pairs_host(6, np.zeros((6, 6), dtype=np.uint8))["state"].shape == (1, 36)  # one board
    # the hooks refuse what the pair-move quench does not run before anything is launched
    lin = {"type": "linear_annealing", "beta_start": 1.0, "beta_end": 3.0}
    seeds = abi.seeds_for(1, 64)
    with pytest.raises(ValueError, match="boards only"):
        mcq_amd.population.anneal_population(6, 1000, "random", lin, seeds, 100, mcmc_type="full_3d", quench="pairs")
    with pytest.raises(ValueError, match="boards only"):
        mcq_amd.heatbath.anneal_heatbath(6, 10, "random", lin, seeds, mcmc_type="full_3d", quench="pairs")
    with pytest.raises(ValueError, match="boards only"):
        mcq_amd.tempering.anneal_tempered(6, 10, "random", lin, seeds, [1.0, 0.5], mcmc_type="full_3d", quench="pairs")
    for call in (lambda: mcq_amd.heatbath.anneal_heatbath(6, 10, "random", lin, seeds, quench="pair"),
                 lambda: mcq_amd.tempering.anneal_tempered(6, 10, "random", lin, seeds, [1.0, 0.5], quench="both"),
                 lambda: mcq_amd.population.anneal_population(6, 1000, "random", lin, seeds, 100, mcmc_type="board", quench="yes"),
                 lambda: mcq_amd.drivers.run_competition(N=6, n_runs=4, n_steps=10, quench="all")):
        with pytest.raises(ValueError, match='"pairs"'):
            call()
    with pytest.raises(ValueError, match="N out of range"):
        mcq_amd.heatbath.anneal_heatbath(40, 10, "random", lin, seeds, quench="pairs")


def test_struct_layout_and_build():
    fields = [f for f, _ in abi.QuenchPairs._fields_]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "mcq.h"\nint main(){printf("%zu %d %d", sizeof(mcq_quench_pairs), MCQ_ABI_VERSION, ' \
        'MCQ_MAX_N_QUENCH_PAIRS);' + "".join(f'printf(" %zu", offsetof(mcq_quench_pairs, {f}));' for f in fields) + "return 0;}"
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(prog)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")], check=True)
        out = subprocess.run([os.path.join(d, "t")], capture_output=True, text=True, check=True).stdout.split()
    assert int(out[0]) == ctypes.sizeof(abi.QuenchPairs) and int(out[1]) == 6 == abi.ABI_VERSION and int(out[2]) == abi.MAX_N_QUENCH_PAIRS
    assert [int(x) for x in out[3:]] == [getattr(abi.QuenchPairs, f).offset for f in fields]
    assert set(abi.QUENCH_PAIRS_DTYPES) | {"state"} == set(qp.FIELDS) == set(quench.FIELDS_PAIRS)
    b = mcq_amd.build
    assert b.PAIRS_SOURCES == [os.path.join(b.CSRC, "mcq_quench_pairs.hip")] and os.path.exists(b.PAIRS_SOURCES[0])
    assert not set(b.PAIRS_SOURCES) & set(b.SOURCES + b.ADDED_SOURCES + b.TEMPER_SOURCES + b.TEMPER3D_SOURCES)
    L = mcq_amd._lib.lib()
    for name in ("mcq_quench_pairs_device", "mcq_quench_pairs_host", "mcq_quench_pairs_last_error"):
        assert hasattr(L, name), name


def test_the_test_sets_make_pair_moves():
    """Not vacuous: on random boards the pair moves fire often, and some run needs several rounds."""
    most = 0
    for N, n, seed in ((4, 40, 2), (5, 24, 3), (6, 16, 4)):
        got = quench.quench_pairs_host(N, qu.random_boards(N, n, seed))
        fired = int((got["n_pair_moves"] > 0).sum())
        print(f"N={N}: {fired} of {n} boards made a pair move, mean energy {got['energy_single'].mean():.2f} -> {got['energy_out'].mean():.2f}, "
              f"most rounds {int(got['n_rounds'].max())}")
        assert 4 * fired >= n, f"N={N}: {fired} of {n}"
        assert (got["energy_out"][got["n_pair_moves"] > 0] < got["energy_single"][got["n_pair_moves"] > 0]).all()
        most = max(most, int(got["n_rounds"].max()))
    assert most >= 3
