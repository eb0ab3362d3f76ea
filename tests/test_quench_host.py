"""CPU-only: the quench rule in host code (mcq_quench_host) and its NumPy restatement (tests/quench_util.py) against the reference's own
conflict counts (tests/golden/conflicts.npz), against each other on every output, the properties of the rule, every refusal, and the
layout of the mcq_quench block."""
import ctypes
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

import mcq_amd
from tests import quench_util as qu

abi = mcq_amd.abi
quench = mcq_amd.quench
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _golden():
    z = np.load(os.path.join(ROOT, "tests", "golden", "conflicts.npz"))
    return z, json.loads(str(z["cases"]))


def test_the_rule_is_the_references_conflict_count():
    """conflicts_for_position for every (i, j, k) and _compute_energy of ~30 boards, captured from the reference."""
    z, cases = _golden()
    assert len(cases) >= 28 and {2, 3, 5, 8, 12, 13, 16, 17, 24, 32, 33, 64} <= {c["N"] for c in cases}
    kinds = {c["what"].split(" N=")[0].split(" of ")[0] for c in cases}
    assert {"random", "latin", "klarner", "final state"} <= kinds
    for c in cases:
        N, key, what = c["N"], c["key"], c["what"]
        h, want, E = z[key + "_heights"], z[key + "_table"].astype(np.int64), int(z[key + "_energy"])
        assert h.shape == (N * N,) and want.shape == (N * N, N) and int(h.max()) < N
        np.testing.assert_array_equal(qu.table(N, h), want, err_msg=f"{what}: the restatement's table a(c, k)")
        assert qu.energy(N, h) == E, what
        got = quench.quench_states_host(N, h, max_passes=1)  # energy_in is the recount of the input whatever the descent does
        assert int(got["energy_in"][0]) == E, what
        held = want[np.arange(N * N), h]
        assert int(held.sum()) == 2 * E, what
        # `conflicts` describes the OUTPUT placement: equal to the reference's counts of the input where nothing moves, and to the
        # restatement's table of the output (pinned to the reference entry for entry just above) in every case
        out = quench.quench_states_host(N, h)
        assert int(out["conflicts"][0].sum()) == 2 * int(out["energy_out"][0]), what
        if int(out["n_moves"][0]) == 0:
            np.testing.assert_array_equal(out["conflicts"][0], held, err_msg=f"{what}: conflicts of an unmoved board")
            np.testing.assert_array_equal(out["state"][0], h)
        np.testing.assert_array_equal(out["conflicts"][0], qu.table(N, out["state"][0])[np.arange(N * N), out["state"][0]], err_msg=what)


def test_conflicts_of_the_input_equal_the_references():
    """Boards that are local minima by the REFERENCE's table come back unmoved after one pass, and their `conflicts` and energies are the
    reference's own numbers."""
    z, cases = _golden()
    unmoved = 0
    for c in cases:
        N, key = c["N"], c["key"]
        h, want = z[key + "_heights"], z[key + "_table"].astype(np.int64)
        held = want[np.arange(N * N), h]
        if (want.min(axis=1) == held).all():  # a local minimum by the REFERENCE's table
            out = quench.quench_states_host(N, h)
            assert int(out["n_moves"][0]) == 0 and int(out["n_passes"][0]) == 1, c["what"]
            np.testing.assert_array_equal(out["conflicts"][0], held, err_msg=c["what"])
            assert int(out["energy_in"][0]) == int(out["energy_out"][0]) == int(z[key + "_energy"])
            unmoved += 1
    assert unmoved >= 3  # the exact klarner boards at least


CASES = [(N, 6 if N <= 16 else 3 if N <= 40 else 1, mp) for N in range(2, 25) for mp in (0, 1, 2)] + \
        [(N, 1, mp) for N, mp in ((31, 0), (32, 2), (33, 0), (48, 1), (63, 2), (64, 0), (65, 1), (100, 2), (96, 0), (127, 1), (128, 2))]


def test_host_code_equals_the_restatement():
    total = 0
    for idx, (N, n, mp) in enumerate(CASES):
        s = qu.random_boards(N, n, 1000 + idx, over=idx % 3 == 1)
        if idx % 4 == 0:
            s[0] = idx % N  # all heights equal
        if idx % 5 == 0:
            s[-1] = 255  # every byte clamped to N - 1: all equal again
        want = qu.quench_many(N, s, mp)
        got = quench.quench_states_host(N, s, max_passes=mp)
        what = f"N={N} max_passes={mp} ({n} boards)"
        qu.assert_equal(got, want, what)
        assert got["state"].dtype == np.uint8 and got["conflicts"].dtype == np.uint16 and got["energy_in"].dtype == np.int32
        assert int(got["state"].max()) < N
        # in place: state_out = state_in
        buf = s.copy()
        q = abi.Quench()
        q.N, q.mode, q.n_chains, q.max_passes = N, abi.MODE_BOARD, n, mp
        q.state_in = q.state_out = buf.ctypes.data
        e_out = np.zeros(n, dtype=np.int32)
        q.energy_out = e_out.ctypes.data  # the other outputs are optional
        mcq_amd._lib.quench_host(q)
        np.testing.assert_array_equal(buf, want["state"], err_msg=f"{what}: in place")
        np.testing.assert_array_equal(e_out, want["energy_out"], err_msg=f"{what}: in place")
        total += n
    assert total >= 300


def test_properties_of_the_rule():
    """Checked with the restatement's table, not with the code under test."""
    for idx, N in enumerate((2, 3, 4, 6, 7, 9, 12, 13, 15, 16, 17, 20, 24, 33, 40, 65)):
        n = 5 if N <= 17 else 2 if N <= 24 else 1
        s = qu.random_boards(N, n, 7000 + idx, over=idx % 2 == 1)
        got = quench.quench_states_host(N, s)
        for r in range(n):
            what = f"N={N} board {r}"
            assert qu.is_local_minimum(N, got["state"][r]), f"{what}: a column of the output has a height with a lower count"
            assert qu.energy(N, s[r]) == int(got["energy_in"][r]) and qu.energy(N, got["state"][r]) == int(got["energy_out"][r]), what
            assert 1 <= int(got["n_passes"][r]) <= int(got["energy_in"][r]) + 1, what
            assert int(got["n_moves"][r]) <= int(got["energy_in"][r]) - int(got["energy_out"][r]), what  # every move drops E by at least 1
        again = quench.quench_states_host(N, got["state"])
        assert (again["n_moves"] == 0).all() and (again["n_passes"] == 1).all(), f"N={N}: an output fed in again"
        np.testing.assert_array_equal(again["state"], got["state"])
        np.testing.assert_array_equal(again["energy_in"], got["energy_out"])
        np.testing.assert_array_equal(again["conflicts"], got["conflicts"])
        # energy_out = energy_in - the sum of the drops, pass by pass: limited runs chained reproduce the unlimited run
        one = quench.quench_states_host(N, s, max_passes=1)
        assert (one["n_passes"] == 1).all() and (one["energy_out"] <= one["energy_in"]).all()
        rest = quench.quench_states_host(N, one["state"])
        np.testing.assert_array_equal(rest["state"], got["state"], err_msg=f"N={N}: one pass, then the rest")
        np.testing.assert_array_equal(rest["energy_in"], one["energy_out"])
        np.testing.assert_array_equal(one["n_moves"] + rest["n_moves"], got["n_moves"])
        want = qu.quench_many(N, s[:1])
        assert int(got["energy_out"][0]) == int(got["energy_in"][0]) - sum(want["drops"][0]) and len(want["drops"][0]) == int(got["n_moves"][0])


def test_zero_energy_boards_come_back_unchanged(golden):
    for N, E in golden.manifest["analytic"]["klarner_exact_board"].items():
        N = int(N)
        assert E == 0
        h = qu.klarner(N)
        got = quench.quench_states_host(N, h)
        np.testing.assert_array_equal(got["state"][0], h, err_msg=f"klarner N={N}")
        assert int(got["energy_in"][0]) == 0 == int(got["energy_out"][0]) and int(got["n_moves"][0]) == 0 and int(got["n_passes"][0]) == 1
        assert not got["conflicts"].any()
        assert qu.energy(N, h) == 0


def test_refusals_name_the_field():
    L = mcq_amd._lib.lib()
    buf = np.zeros((4, 36), dtype=np.uint8)

    def block(**kw):
        q = abi.Quench()
        q.N, q.mode, q.n_chains, q.max_passes = 6, abi.MODE_BOARD, 4, 0
        q.state_in = q.state_out = buf.ctypes.data
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    refused = ((dict(mode=abi.MODE_FULL3D), b"mode"), (dict(mode=7), b"mode"), (dict(N=1), b"N out of range"), (dict(N=129), b"N out of range"),
               (dict(N=-3), b"N out of range"), (dict(n_chains=0), b"n_chains"), (dict(n_chains=-1), b"n_chains"), (dict(n_chains=1 << 31), b"n_chains"),
               (dict(max_passes=-1), b"max_passes"), (dict(state_in=None), b"state_in"), (dict(state_out=None), b"state_out"))
    for kw, msg in refused:
        for fn in (L.mcq_quench_host, lambda q: L.mcq_quench_device(q, None)):  # the device entry point refuses before any launch: no GPU here
            assert fn(ctypes.byref(block(**kw))) == abi.EINVAL, kw
            assert msg in L.mcq_quench_last_error(), (kw, L.mcq_quench_last_error())
    assert L.mcq_quench_host(None) == abi.EINVAL and L.mcq_quench_device(None, None) == abi.EINVAL
    assert L.mcq_quench_host(ctypes.byref(block())) == abi.OK
    with pytest.raises(ValueError, match="N out of range"):
        quench.quench_states_host(200, np.zeros((2, 40000), dtype=np.uint8))
    with pytest.raises(ValueError, match="max_passes"):
        quench.quench_states_host(6, buf, max_passes=-2)
    with pytest.raises(ValueError, match="n_chains"):
        quench.quench_states_host(6, np.zeros((0, 36), dtype=np.uint8))
    with pytest.raises(ValueError, match="final_state layout"):
        quench.quench_states_host(6, np.zeros((2, 35), dtype=np.uint8))
    assert quench.quench_states_host(6, np.zeros((6, 6), dtype=np.uint8))["state"].shape == (1, 36)  # one board
    # the hooks refuse what the quench does not run before anything is launched
    lin = {"type": "linear_annealing", "beta_start": 1.0, "beta_end": 3.0}
    with pytest.raises(ValueError, match="boards only"):
        mcq_amd.population.anneal_population(6, 1000, "random", lin, abi.seeds_for(1, 64), 100, mcmc_type="full_3d", quench=True)


def test_quench_struct_layout_and_build():
    fields = [f for f, _ in abi.Quench._fields_]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "mcq.h"\nint main(){printf("%zu %d", sizeof(mcq_quench), MCQ_ABI_VERSION);' + \
        "".join(f'printf(" %zu", offsetof(mcq_quench, {f}));' for f in fields) + "return 0;}"
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(prog)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")], check=True)
        out = subprocess.run([os.path.join(d, "t")], capture_output=True, text=True, check=True).stdout.split()
    assert int(out[0]) == ctypes.sizeof(abi.Quench) and int(out[1]) == 6 == abi.ABI_VERSION
    assert [int(x) for x in out[2:]] == [getattr(abi.Quench, f).offset for f in fields]
    L = mcq_amd._lib.lib()
    assert os.path.join(mcq_amd.build.CSRC, "mcq_quench.hip") in mcq_amd.build.SOURCES
    for name in ("mcq_quench_device", "mcq_quench_host", "mcq_quench_last_error"):
        assert hasattr(L, name), name
