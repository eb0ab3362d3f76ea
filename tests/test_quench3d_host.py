"""CPU-only: the full_3d quench rule in host code (mcq_quench3d_host) and its NumPy restatement (tests/quench3d_util.py) against the
reference's own conflict counts (tests/golden/conflicts_3d.npz), against each other on every output, the invariants of the rule, the
oracle's end states, every refusal, and the layout of the mcq_quench3d block."""
import ctypes
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

import mcq_amd
from tests import quench3d_util as qu

abi = mcq_amd.abi
quench = mcq_amd.quench
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIN = {"type": "linear_annealing", "beta_start": 1.0, "beta_end": 3.0}


def _golden():
    z = np.load(os.path.join(ROOT, "tests", "golden", "conflicts_3d.npz"))
    return z, json.loads(str(z["cases"]))


def test_the_rule_is_the_references_conflict_count():
    """conflicts_for_queen(q, t) and _compute_energy of ~30 placements of State3DQueens, captured from the reference: the restatement
    entry for entry, and the host code's recount and conflict map."""
    z, cases = _golden()
    assert len(cases) >= 25 and {2, 3, 4, 5, 6, 8, 12, 16, 20, 24, 32} <= {c["N"] for c in cases}
    kinds = {c["what"].split(" N=")[0].split(" of ")[0] for c in cases}
    assert {"random", "latin", "klarner", "final state"} <= kinds
    assert any(c["Q"] != c["N"] ** 2 for c in cases) and any(c["Q"] == c["N"] ** 3 - 1 for c in cases) and any(c["Q"] == 2 for c in cases)
    assert set(z.files) == {"cases"} | {c["key"] + s for c in cases for s in ("_queens", "_cells", "_table", "_energy")}  # data only
    for c in cases:
        N, Q, key, what = c["N"], c["Q"], c["key"], c["what"]
        queens, cells, want, E = z[key + "_queens"], z[key + "_cells"].astype(np.int64), z[key + "_table"].astype(np.int64), int(z[key + "_energy"])
        assert queens.shape == (Q, 3) and want.shape == (Q, len(cells)) and int(queens.max()) < N
        assert (len(cells) == N ** 3) == c["all_cells"] == (N <= 8)
        own = (queens[:, 0].astype(np.int64) * N + queens[:, 1]) * N + queens[:, 2]
        assert np.isin(own, cells).all(), f"{what}: every occupied cell is recorded"
        pos = np.stack([cells // (N * N), (cells // N) % N, cells % N], axis=1)
        zq = qu.clamp(N, queens)
        for q in range(Q):
            np.testing.assert_array_equal(qu.counts(N, zq, q, pos), want[q], err_msg=f"{what}: the restatement's a({q}, t)")
        assert qu.energy(N, queens) == E == qu.pairwise_energy(N, queens), what
        held = want[np.arange(Q), np.searchsorted(cells, own)]  # the reference's a(q, pos(q))
        assert int(held.sum()) == 2 * E, what
        np.testing.assert_array_equal(qu.held(N, zq), held, err_msg=what)
        got = quench.quench_queens_host(N, queens.reshape(1, -1), Q=Q, max_passes=1)  # energy_in is the recount whatever the descent does
        assert int(got["energy_in"][0]) == E and int(got["flags"][0]) == 0, what
        out = quench.quench_queens_host(N, queens.reshape(1, -1), Q=Q)
        assert int(out["conflicts"][0].sum()) == 2 * int(out["energy_out"][0]), what
        # a local minimum by the REFERENCE's table (where it covers every cell) comes back unmoved with the reference's own counts
        if c["all_cells"]:
            free = np.ones((Q, N ** 3), dtype=bool)
            free[:, own] = False
            free[np.arange(Q), own] = True
            minimum = bool((np.where(free, want, 1 << 20).min(axis=1) == held).all())
            assert minimum == (int(out["n_moves"][0]) == 0), what
        if int(out["n_moves"][0]) == 0:
            assert int(out["n_passes"][0]) == 1
            np.testing.assert_array_equal(out["conflicts"][0], held, err_msg=f"{what}: conflicts of an unmoved placement")
            np.testing.assert_array_equal(out["state"][0], queens.reshape(-1))
        np.testing.assert_array_equal(out["conflicts"][0], qu.held(N, qu.clamp(N, out["state"][0])), err_msg=what)


# (N, Q or None = N^2, chains, max_passes)
CASES = [(N, None, 4 if N <= 8 else 2, 0) for N in range(2, 13)] + \
        [(N, None, 2, mp) for N in (3, 5, 8, 11) for mp in (1, 2)] + \
        [(16, 40, 2, 0), (19, 60, 2, 0), (20, 60, 2, 0), (32, 40, 1, 0), (32, 24, 1, 1), (19, 45, 1, 2), (20, 45, 1, 1)] + \
        [(2, 2, 4, 0), (3, 2, 4, 0), (7, 2, 3, 0), (2, 7, 3, 0), (3, 26, 3, 0), (4, 63, 2, 0), (5, 124, 1, 0), (4, 63, 2, 1)] + \
        [(4, 10, 3, 0), (6, 50, 3, 0), (6, 100, 2, 2), (9, 30, 3, 0), (12, 100, 2, 0), (12, 300, 1, 1), (5, 3, 4, 0)]


def test_host_code_equals_the_restatement():
    total = 0
    for idx, (N, Q, n, mp) in enumerate(CASES):
        s = qu.random_placements(N, n, 2000 + idx, Q=Q, over=idx % 3 == 1)  # over: bytes >= N, clamped back
        Qn = N * N if Q is None else Q
        want = qu.quench_many(N, s, Q=Q, max_passes=mp)
        got = quench.quench_queens_host(N, s, Q=Q, max_passes=mp)
        what = f"N={N} Q={Qn} max_passes={mp} ({n} placements)"
        qu.assert_equal(got, want, what)
        assert got["state"].dtype == np.uint8 and got["conflicts"].dtype == np.uint16 and got["energy_in"].dtype == np.int32
        assert got["state"].shape == (n, 3 * Qn) and got["conflicts"].shape == (n, Qn) and int(got["state"].max()) < N
        assert not got["flags"].any()
        if mp:
            assert (got["n_passes"] <= mp).all()
        # the [n][Q][3] form is the same call
        qu.assert_equal(quench.quench_queens_host(N, s.reshape(n, Qn, 3), Q=Q, max_passes=mp), want, what + " as [n][Q][3]")
        # in place: state_out = state_in, and only energy_out asked for -- the other outputs are optional
        buf = s.copy()
        q = abi.Quench3D()
        q.N, q.n_queens, q.n_chains, q.max_passes = N, 0 if Q is None else Q, n, mp
        q.state_in = q.state_out = buf.ctypes.data
        e_out = np.zeros(n, dtype=np.int32)
        q.energy_out = e_out.ctypes.data
        mcq_amd._lib.quench3d_host(q)
        np.testing.assert_array_equal(buf, want["state"], err_msg=f"{what}: in place")
        np.testing.assert_array_equal(e_out, want["energy_out"], err_msg=f"{what}: in place")
        # no optional output at all
        buf2, o2 = s.copy(), np.zeros_like(s)
        q2 = abi.Quench3D()
        q2.N, q2.n_queens, q2.n_chains, q2.max_passes, q2.state_in, q2.state_out = N, Qn, n, mp, buf2.ctypes.data, o2.ctypes.data
        mcq_amd._lib.quench3d_host(q2)
        np.testing.assert_array_equal(o2, want["state"], err_msg=f"{what}: placements only")
        np.testing.assert_array_equal(buf2, s)  # out of place: the input is untouched
        total += n
    assert total >= 100
    assert quench.quench_queens_host(6, qu.random_placements(6, 1, 1)[0])["state"].shape == (1, 108)  # one placement
    assert quench.quench_queens_host(6, qu.random_placements(6, 1, 1).reshape(36, 3), conflicts=False).keys() == set(qu.FIELDS) - {"conflicts"}


def test_repeated_cells_are_flagged_and_nothing_moves():
    for idx, (N, Q) in enumerate(((2, 2), (3, None), (6, None), (6, 20), (12, None), (19, 50), (20, 50), (5, 124), (12, 1727))):
        Qn = N * N if Q is None else Q
        s = qu.random_placements(N, 3, 3000 + idx, Q=Q).reshape(3, Qn, 3)
        s[0, Qn - 1] = s[0, 0]  # two queens in one cell
        s[1, :, :] = 255  # every byte clamped: all queens in the corner cell
        want = qu.quench_many(N, s, Q=Q)
        got = quench.quench_queens_host(N, s, Q=Q)
        what = f"N={N} Q={Qn}"
        qu.assert_equal(got, want, what)
        assert list(got["flags"]) == [abi.QUENCH3D_REPEATED, abi.QUENCH3D_REPEATED, 0], what
        for r in (0, 1):
            assert int(got["n_moves"][r]) == 0 == int(got["n_passes"][r]) and int(got["energy_in"][r]) == int(got["energy_out"][r]), what
            np.testing.assert_array_equal(got["state"][r], np.minimum(s[r], N - 1).reshape(-1), err_msg=f"{what}: the clamped input")
            assert int(got["conflicts"][r].sum()) == 2 * int(got["energy_in"][r])
        assert int(got["energy_in"][1]) == Qn * (Qn - 1) // 2 and (got["conflicts"][1] == Qn - 1).all(), what  # every pair shares the cell
        if Qn <= 150:
            assert int(got["energy_in"][0]) == qu.pairwise_energy(N, s[0]), what
        # the unflagged chain next to them is quenched as if alone
        alone = quench.quench_queens_host(N, s[2:], Q=Q)
        for k in qu.FIELDS:
            np.testing.assert_array_equal(alone[k][0], got[k][2], err_msg=f"{what}: {k}")


def test_invariants_of_the_rule():
    total = 0
    for idx, (N, Q, n) in enumerate(((2, None, 20), (2, 3, 20), (3, None, 40), (4, None, 40), (4, 30, 20), (5, None, 40), (6, None, 40), (6, 12, 20),
                                     (8, None, 30), (8, 200, 10), (10, None, 16), (12, None, 16), (13, 60, 8), (16, 256, 4), (19, 100, 4),
                                     (20, 100, 4), (24, 64, 2), (32, 96, 2))):
        Qn = N * N if Q is None else Q
        s = qu.random_placements(N, n, 7000 + idx, Q=Q, over=idx % 2 == 1)
        got = quench.quench_queens_host(N, s, Q=Q)
        what = f"N={N} Q={Qn}"
        assert (got["energy_out"] <= got["energy_in"]).all() and not got["flags"].any(), what
        unchanged = (got["state"] == np.minimum(s, N - 1)).all(axis=1)
        np.testing.assert_array_equal(got["n_moves"] == 0, unchanged, err_msg=what)
        np.testing.assert_array_equal(got["n_moves"] == 0, got["n_passes"] == 1, err_msg=what)
        np.testing.assert_array_equal(got["conflicts"].sum(axis=1), 2 * got["energy_out"], err_msg=what)
        assert ((got["n_passes"] >= 1) & (got["n_passes"] <= got["energy_in"] + 1)).all(), what
        assert (got["n_moves"] <= got["energy_in"] - got["energy_out"]).all(), what  # every move drops E by at least 1
        for r in range(n):
            assert not qu.is_repeated(N, got["state"][r]), f"{what}: chain {r} has a repeated cell in the output"
        for r in range(min(n, 4)):
            assert qu.pairwise_energy(N, got["state"][r]) == int(got["energy_out"][r]), f"{what}: chain {r}"
            assert qu.pairwise_energy(N, s[r]) == int(got["energy_in"][r]), f"{what}: chain {r}"
        if N <= 12:
            assert qu.is_local_minimum(N, got["state"][0]), f"{what}: a queen of the output has a free cell with a lower count"
        again = quench.quench_queens_host(N, got["state"], Q=Q)
        assert (again["n_moves"] == 0).all() and (again["n_passes"] == 1).all(), f"{what}: an output fed in again"
        np.testing.assert_array_equal(again["state"], got["state"])
        np.testing.assert_array_equal(again["energy_in"], got["energy_out"])
        np.testing.assert_array_equal(again["conflicts"], got["conflicts"])
        # limited runs chained reproduce the unlimited run
        one = quench.quench_queens_host(N, s, Q=Q, max_passes=1)
        assert (one["n_passes"] == 1).all() and (one["energy_out"] <= one["energy_in"]).all()
        rest = quench.quench_queens_host(N, one["state"], Q=Q)
        np.testing.assert_array_equal(rest["state"], got["state"], err_msg=f"{what}: one pass, then the rest")
        np.testing.assert_array_equal(rest["energy_in"], one["energy_out"])
        np.testing.assert_array_equal(one["n_moves"] + rest["n_moves"], got["n_moves"])
        total += n
    assert total >= 300


def test_zero_energy_placements_come_back_unchanged():
    for N in (11, 13, 17, 23):  # gcd(N, 210) = 1: k = (3 i + 5 j) mod N has no attacking pair
        i, j = np.indices((N, N))
        s = np.stack([i.ravel(), j.ravel(), ((3 * i + 5 * j) % N).ravel()], axis=1).astype(np.uint8)
        got = quench.quench_queens_host(N, s)
        assert qu.energy(N, s) == 0 == int(got["energy_in"][0]) == int(got["energy_out"][0])
        assert int(got["n_moves"][0]) == 0 and int(got["n_passes"][0]) == 1 and not got["conflicts"].any()
        np.testing.assert_array_equal(got["state"][0], s.reshape(-1))


def test_energy_in_is_the_oracles_final_energy():
    """End states of full_3d oracle chains: the recount equals what the oracle accumulated step by step."""
    from oracle import oracle

    for N, Q, steps in ((3, None, 300), (6, None, 400), (8, None, 400), (12, None, 500), (6, 100, 300), (12, 60, 300), (20, None, 200)):
        n = 16
        p = abi.make_params(N, steps, "random", LIN, n, mcmc_type="full_3d", Q=Q)
        res = oracle.run(p, abi.seeds_for(11, n), trace=False, n_threads=4)
        for which in ("final", "best"):
            got = quench.quench_queens_host(N, res[which + "_state"], Q=Q)
            np.testing.assert_array_equal(got["energy_in"], res[which + "_energy"], err_msg=f"N={N} Q={Q}: energy_in of {which}_state")
            assert (got["energy_out"] <= got["energy_in"]).all() and not got["flags"].any()


def test_refusals_name_the_field():
    L = mcq_amd._lib.lib()
    buf = np.zeros((4, 3 * 215), dtype=np.uint8)  # (room for the largest Q a block below asks for)

    def block(**kw):
        q = abi.Quench3D()
        q.N, q.n_queens, q.n_chains, q.max_passes = 6, 0, 4, 0
        q.state_in = q.state_out = buf.ctypes.data
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    refused = ((dict(N=1), b"N out of range [2, 32]"), (dict(N=-3), b"N out of range"), (dict(N=33), b"stops at N = 32"), (dict(N=64), b"stops at N = 32"),
               (dict(N=65), b"N out of range [2, 32]"), (dict(n_queens=1), b"n_queens"), (dict(n_queens=-2), b"n_queens"), (dict(n_queens=216), b"n_queens"),
               (dict(n_queens=217), b"N^3 - 1 = 215"), (dict(n_chains=0), b"n_chains"), (dict(n_chains=-1), b"n_chains"), (dict(n_chains=1 << 31), b"n_chains"),
               (dict(max_passes=-1), b"max_passes"), (dict(state_in=None), b"state_in"), (dict(state_out=None), b"state_out"))
    for kw, msg in refused:
        for fn in (L.mcq_quench3d_host, lambda q: L.mcq_quench3d_device(q, None)):  # the device entry point refuses before any launch: no GPU here
            assert fn(ctypes.byref(block(**kw))) == abi.EINVAL, kw
            assert msg in L.mcq_quench3d_last_error(), (kw, L.mcq_quench3d_last_error())
    assert L.mcq_quench3d_host(None) == abi.EINVAL and L.mcq_quench3d_device(None, None) == abi.EINVAL
    assert b"NULL" in L.mcq_quench3d_last_error()
    assert L.mcq_quench3d_host(ctypes.byref(block())) == abi.OK
    assert L.mcq_quench3d_host(ctypes.byref(block(n_queens=215))) == abi.OK  # N^3 - 1: all queens in one cell here, flagged
    # a message of its own: the board quench's is untouched by these calls
    L.mcq_quench_host(None)
    before = L.mcq_quench_last_error()
    L.mcq_quench3d_host(ctypes.byref(block(N=40)))
    assert L.mcq_quench_last_error() == before and b"stops at N = 32" in L.mcq_quench3d_last_error()
    with pytest.raises(ValueError, match="N out of range"):
        quench.quench_queens_host(40, np.zeros((2, 4800), dtype=np.uint8))
    with pytest.raises(ValueError, match="max_passes"):
        quench.quench_queens_host(6, buf[:, :108], max_passes=-2)
    with pytest.raises(ValueError, match="n_chains"):
        quench.quench_queens_host(6, np.zeros((0, 108), dtype=np.uint8))
    with pytest.raises(ValueError, match="n_queens"):
        quench.quench_queens_host(3, np.zeros((2, 81), dtype=np.uint8), Q=27)
    with pytest.raises(ValueError, match="final_state layout of full_3d"):
        quench.quench_queens_host(6, np.zeros((2, 107), dtype=np.uint8))
    # mcq_quench still refuses full_3d, and the hooks still refuse it before anything is launched
    q = abi.Quench()
    q.N, q.mode, q.n_chains, q.max_passes = 6, abi.MODE_FULL3D, 4, 0
    q.state_in = q.state_out = buf.ctypes.data
    assert L.mcq_quench_host(ctypes.byref(q)) == abi.EINVAL and b"boards only" in L.mcq_quench_last_error()
    with pytest.raises(ValueError, match="boards only"):
        mcq_amd.population.anneal_population(6, 1000, "random", LIN, abi.seeds_for(1, 64), 100, mcmc_type="full_3d", quench=True)


def test_quench3d_struct_layout_and_build():
    fields = [f for f, _ in abi.Quench3D._fields_]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "mcq.h"\nint main(){printf("%zu %d %d %d", sizeof(mcq_quench3d), MCQ_ABI_VERSION, ' \
        'MCQ_MAX_N_QUENCH3D, MCQ_QUENCH3D_REPEATED);' + "".join(f'printf(" %zu", offsetof(mcq_quench3d, {f}));' for f in fields) + "return 0;}"
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(prog)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")], check=True)
        out = subprocess.run([os.path.join(d, "t")], capture_output=True, text=True, check=True).stdout.split()
    assert int(out[0]) == ctypes.sizeof(abi.Quench3D) and int(out[1]) == 6 == abi.ABI_VERSION
    assert int(out[2]) == abi.MAX_N_QUENCH3D == 32 and int(out[3]) == abi.QUENCH3D_REPEATED == 1
    assert [int(x) for x in out[4:]] == [getattr(abi.Quench3D, f).offset for f in fields]
    assert set(abi.QUENCH3D_DTYPES) < set(fields)
    L = mcq_amd._lib.lib()
    assert os.path.join(mcq_amd.build.CSRC, "mcq_quench3d.hip") in mcq_amd.build.SOURCES and len(mcq_amd.build.SOURCES) == 6
    for name in ("mcq_quench3d_device", "mcq_quench3d_host", "mcq_quench3d_last_error"):
        assert hasattr(L, name), name
    for name in ("quench_queens", "quench_queens_device", "quench_queens_host"):
        assert callable(getattr(quench, name)), name
