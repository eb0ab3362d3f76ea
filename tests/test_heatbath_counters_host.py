"""CPU-only: the identity the counter form of the heat-bath sweep rests on (tests/heatbath_counters_util.py against tests/quench_util.py and
the reference's conflict counts), and the interface of the form: the header, the library's export, the constants, the Python arguments
and every refusal that is made before a GPU is touched."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import mcq_amd
from tests import heatbath_counters_util as cu
from tests import quench_util as qu

abi = mcq_amd.abi
heatbath = mcq_amd.heatbath
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIN = {"type": "linear_annealing", "beta_start": 1.0, "beta_end": 3.0}


def _boards(N):
    diag, rows = cu.special_boards(N)
    over = qu.random_boards(N, 1, 900 + N, over=True)[0]
    over[:3] = (N, 255, 128)  # bytes >= N whatever the draw
    return {"random": qu.random_boards(N, 1, N)[0], "random 2": qu.random_boards(N, 1, 50 + N)[0], "all equal": np.full(N * N, N // 2, dtype=np.uint8),
            "(i + j) mod N": diag, "h = i": rows, "bytes >= N": over, "all 255": np.full(N * N, 255, dtype=np.uint8)}


@pytest.mark.parametrize("N", range(2, 17))
def test_counters_give_the_quench_rules_table(N):
    for what, board in _boards(N).items():
        h = qu.clamp(N, board)
        cnt = cu.build(N, board)
        np.testing.assert_array_equal(cu.table(N, cnt, h), qu.table(N, board), err_msg=f"N={N}, {what}")
        assert 0 <= cnt.min() and cnt.max() <= N, f"N={N}, {what}: a counter of {cnt.max()}"
        assert cnt.sum() == 12 * N * N  # every queen on 12 lines
    for what in ("(i + j) mod N", "h = i", "all equal"):
        assert cu.build(N, _boards(N)[what]).max() == N, f"N={N}, {what}: no line is full"
    assert cu.n_lines(N) == 26 * N * N - 18 * N + 4


def test_counters_give_the_references_counts():
    z = np.load(os.path.join(ROOT, "tests", "golden", "conflicts.npz"))
    cases = [c for c in json.loads(str(z["cases"])) if c["N"] <= abi.MAX_N_HEATBATH_COUNTERS]
    assert len(cases) >= 5
    for c in cases:
        N, key = c["N"], c["key"]
        h = qu.clamp(N, z[key + "_heights"])
        np.testing.assert_array_equal(cu.table(N, cu.build(N, h), h), z[key + "_table"].astype(np.int64), err_msg=c["what"])


@pytest.mark.parametrize("N", range(2, 17))
def test_incremental_updates_equal_a_rebuild(N):
    rs = np.random.RandomState(N)
    board = qu.random_boards(N, 1, 7 * N, over=True)[0]
    h = qu.clamp(N, board).copy()
    cnt = cu.build(N, board)
    for step in range(200):
        c = int(rs.randint(N * N))
        k = int((h[c] + 1 + rs.randint(N - 1)) % N)  # any height but the one it holds
        touched = cu.change(N, cnt, h, c, k)
        assert len(set(touched)) == 24, f"N={N}: a changed height touched {len(set(touched))} distinct counters"
        assert 0 <= cnt.min() and cnt.max() <= N
        if step % 50 == 49:
            np.testing.assert_array_equal(cnt, cu.build(N, h), err_msg=f"N={N} after {step + 1} changes")
    np.testing.assert_array_equal(cu.table(N, cnt, h), qu.table(N, h), err_msg=f"N={N}: the table after 200 changes")


def test_header_library_and_constants():
    text = open(os.path.join(ROOT, "include", "mcq.h")).read()
    assert re.search(r"int\s+mcq_heatbath_counters_device\s*\(\s*const\s+mcq_heatbath\s*\*\s*q\s*,\s*void\s*\*\s*hip_stream\s*\)\s*;", text)
    m = re.search(r"#define\s+MCQ_MAX_N_HEATBATH_COUNTERS\s+(\d+)", text)
    assert m and int(m.group(1)) == abi.MAX_N_HEATBATH_COUNTERS == 16
    L = mcq_amd._lib.lib()
    assert hasattr(L, "mcq_heatbath_counters_device") and callable(mcq_amd._lib.heatbath_counters_device)
    assert heatbath.FORMS == ("lines", "counters")
    assert len(mcq_amd.build.SOURCES) == 6 and len(mcq_amd.build.ADDED_SOURCES) == 1 and abi.ABI_VERSION == 6 == L.mcq_abi_version()
    for fn in (heatbath.heatbath_device, heatbath.heatbath_states, heatbath.anneal_heatbath):
        names = fn.__code__.co_varnames[: fn.__code__.co_argcount]
        assert "form" in names and fn.__defaults__[names.index("form") - len(names)] == "lines", fn.__name__
    drv = mcq_amd.drivers.run_competition
    names = drv.__code__.co_varnames[: drv.__code__.co_argcount]
    assert drv.__defaults__[names.index("heatbath_form") - len(names)] == "lines"
    for fn in (heatbath.heatbath_queens, heatbath.heatbath_queens_device, heatbath.heatbath_queens_host, heatbath.heatbath_states_host):
        assert "form" not in fn.__code__.co_varnames[: fn.__code__.co_argcount], fn.__name__


def test_the_entry_point_refuses_before_any_launch():
    """No GPU here: the device entry point returns before it launches anything."""
    L = mcq_amd._lib.lib()
    seeds, tab = np.zeros(4, dtype=np.uint32), abi.heatbath_table([1.0, 2.0])

    def block(edge, **kw):
        N = edge
        buf = np.zeros((4, N * N), dtype=np.uint8)
        q = abi.Heatbath()
        q.N, q.mode, q.n_chains, q.n_sweeps, q.first_sweep, q.table_len = N, abi.MODE_BOARD, 4, 2, 0, tab.shape[1]
        q.seeds, q.table = seeds.ctypes.data, tab.ctypes.data
        q.state_in = q.state_out = buf.ctypes.data
        for k, v in kw.items():
            setattr(q, k, v)
        return q, buf

    for N in (17, 24, 128):
        q, _keep = block(N)
        assert L.mcq_heatbath_counters_device(ctypes.byref(q), None) == abi.EINVAL
        msg = L.mcq_heatbath_last_error()
        assert b"16" in msg and b"mcq_heatbath_device" in msg, msg
    # the refusals of mcq_heatbath_device, with their messages
    for kw, msg in ((dict(mode=abi.MODE_FULL3D), b"boards only"), (dict(N=1), b"N out of range"), (dict(N=129), b"N out of range"), (dict(n_chains=0), b"n_chains"),
                    (dict(n_sweeps=-1), b"n_sweeps"), (dict(first_sweep=-1), b"first_sweep"), (dict(table_len=513), b"table_len"), (dict(seeds=None), b"seeds"),
                    (dict(table=None), b"table"), (dict(state_in=None), b"state_in"), (dict(state_out=None), b"state_out")):
        q, _keep = block(6, **kw)
        assert L.mcq_heatbath_counters_device(ctypes.byref(q), None) == abi.EINVAL, kw
        assert msg in L.mcq_heatbath_last_error(), (kw, L.mcq_heatbath_last_error())
    assert L.mcq_heatbath_counters_device(None, None) == abi.EINVAL
    q, _keep = block(16, n_chains=0)  # N = 16 itself is not what is refused
    assert L.mcq_heatbath_counters_device(ctypes.byref(q), None) == abi.EINVAL and b"n_chains" in L.mcq_heatbath_last_error()


def test_python_refuses_before_any_gpu_call():
    """None of these reaches the GPU: there is none here."""
    boards, seeds = qu.random_boards(6, 64, 1), abi.seeds_for(42, 64)
    big = np.zeros((2, 17 * 17), dtype=np.uint8)
    with pytest.raises(ValueError, match="Unknown form"):
        heatbath.heatbath_device(6, boards, seeds, [1.0], form="bytes")
    with pytest.raises(ValueError, match="Unknown form"):
        heatbath.heatbath_states(6, boards, seeds, [1.0], form="auto")
    with pytest.raises(ValueError, match="N <= 16"):
        heatbath.heatbath_device(17, big, [1, 2], [1.0], form="counters")
    with pytest.raises(ValueError, match="N <= 16"):
        heatbath.heatbath_states(17, big, [1, 2], [1.0], form="counters")
    with pytest.raises(ValueError, match="N <= 16"):
        heatbath.anneal_heatbath(17, 10, "random", LIN, seeds, form="counters")
    with pytest.raises(ValueError, match="Unknown form"):
        heatbath.anneal_heatbath(6, 10, boards, LIN, seeds, form="Lines")
    for form in ("counters", "bytes"):
        with pytest.raises(ValueError, match='one form "lines"'):
            heatbath.anneal_heatbath(6, 10, "random", LIN, seeds, mcmc_type="full_3d", form=form)
    with pytest.raises(ValueError, match="Unknown form"):
        mcq_amd.drivers.run_competition(N=6, n_runs=16, heatbath_sweeps=4, heatbath_form="bytes")
    with pytest.raises(ValueError, match="N <= 16"):
        mcq_amd.drivers.run_competition(N=17, n_runs=16, heatbath_sweeps=4, heatbath_form="counters")
    # the refusals that were there stay in front of nothing new: a good form goes on to them
    with pytest.raises(ValueError, match="one schedule"):
        heatbath.anneal_heatbath(6, 10, boards, [LIN, LIN], seeds, form="counters")
    with pytest.raises(ValueError, match="contiguous uint8 tensor on the GPU"):
        heatbath.heatbath_device(6, boards, seeds, [1.0], form="counters")
