"""CPU-only: the interface of the counter form of the tempered board sweep (mcq_temper_counters_device, form="counters") -- the header,
the library's export, the constants, the LDS arithmetic, the Python arguments, which entry point a form reaches, and every refusal that
is made before a GPU is touched."""
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import mcq_amd
from tests import quench_util as qu

abi = mcq_amd.abi
heatbath = mcq_amd.heatbath
tempering = mcq_amd.tempering
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIN = {"type": "linear_annealing", "beta_start": 1.0, "beta_end": 3.0}


def test_header_library_and_constants():
    text = open(os.path.join(ROOT, "include", "mcq.h")).read()
    assert re.search(r"int\s+mcq_temper_counters_device\s*\(\s*const\s+mcq_temper\s*\*\s*q\s*,\s*void\s*\*\s*hip_stream\s*\)\s*;", text)
    prog = '#include <stdio.h>\n#include "mcq.h"\nint main(){printf("%d %d %zu", MCQ_MAX_N_TEMPER_COUNTERS, MCQ_ABI_VERSION, sizeof(mcq_temper));return 0;}'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(prog)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")], check=True)
        out = subprocess.run([os.path.join(d, "t")], capture_output=True, text=True, check=True).stdout.split()
    assert int(out[0]) == abi.MAX_N_TEMPER_COUNTERS == 16
    assert int(out[1]) == 6 == abi.ABI_VERSION and int(out[2]) == ctypes.sizeof(abi.Temper)  # the block is mcq_temper_device's, unchanged
    L = mcq_amd._lib.lib()
    assert L.mcq_abi_version() == 6
    assert hasattr(L, "mcq_temper_counters_device") and callable(mcq_amd._lib.temper_counters_device)
    assert tempering.FORMS is heatbath.FORMS and tempering.FORMS == ("lines", "counters")
    for fn in (tempering.temper_device, tempering.temper_states, tempering.anneal_tempered):
        names = fn.__code__.co_varnames[: fn.__code__.co_argcount]
        assert "form" in names and fn.__defaults__[names.index("form") - len(names)] == "lines", fn.__name__
    for fn in (tempering.temper_states_host, tempering.temper_queens, tempering.temper_queens_device, tempering.temper_queens_host):
        assert "form" not in fn.__code__.co_varnames[: fn.__code__.co_argcount], fn.__name__


def test_the_build_lists_are_what_they_were():
    built = mcq_amd.build.TEMPER_SOURCES
    assert built == [os.path.join(mcq_amd.build.CSRC, "mcq_temper.hip")] and all(os.path.exists(f) for f in built)
    assert len(mcq_amd.build.SOURCES) == 6 and len(mcq_amd.build.ADDED_SOURCES) == 1
    assert "mcq_temper_counters_kernel" in open(built[0]).read()  # the kernel stands next to mcq_temper_kernel
    assert os.path.join(mcq_amd.build.CSRC, "mcq_columns.h") in mcq_amd.build.HEADERS  # where both counter kernels read the layout
    t = os.path.getmtime(mcq_amd.build.SO)
    assert all(os.path.getmtime(f) <= t for f in built + mcq_amd.build.HEADERS) or mcq_amd.build.stale()  # stale() sees the file


def test_lds_bytes_stay_within_a_workgroup():
    assert abi.temper_counters_lds_bytes(16, 16, 512) == 154816 == 16 * 7616 + 4 * 16 * 512 + 12 * 16
    assert abi.temper_counters_lds_bytes(16, 16) == 154816  # the longest table is the default
    regions = {8: 1856, 12: 4288, 16: 7616}
    largest = 0
    for N in range(2, 17):
        NP = 8 if N <= 8 else 12 if N <= 12 else 16
        for R in (2, 4, 8, 16):
            for D in range(1, 513):
                b = abi.temper_counters_lds_bytes(N, R, D)
                assert b == (2 if R == 2 else 1) * (R * regions[NP] + 4 * R * D + 12 * R), (N, R, D)  # (R = 2: two ladders share a wavefront)
                largest = max(largest, b)
    assert largest == 154816 <= abi.MAX_TEMPER_LDS == 160 * 1024
    for N, R in ((17, 4), (1, 4), (12, 3), (12, 32)):
        with pytest.raises(ValueError):
            abi.temper_counters_lds_bytes(N, R, 10)


def _block_maker(N=6, n=8, R=4, K=2):
    buf, seeds = np.zeros((n, N * N), dtype=np.uint8), np.zeros(n, dtype=np.uint32)
    T, X = abi.temper_tables([1.0, 2.0, 2.5], [0.5, 1.0, 1.5, 2.0][:R] if R <= 4 else list(np.linspace(0.5, 2.0, R)), K, 1)
    keep = (buf, seeds, T, X)

    def block(**kw):
        q = tempering._block(N, n, 3, 1, R, K, T.shape[2], X.shape[2])
        q.seeds, q.table, q.swap_table = seeds.ctypes.data, T.ctypes.data, X.ctypes.data
        q.state_in = q.state_out = buf.ctypes.data
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    return block, keep


def test_the_entry_point_refuses_n_above_16_before_any_launch():
    """No GPU here and a NULL stream: the entry point returns before it launches anything."""
    L = mcq_amd._lib.lib()
    for N in (17, 24, 64, 128):
        block, keep = _block_maker(N=N)
        before = keep[0].copy()
        assert L.mcq_temper_counters_device(ctypes.byref(block()), None) == abi.EINVAL, N
        msg = L.mcq_temper_last_error()
        assert b"16" in msg and f"N = {N}".encode() in msg and b"mcq_temper_device" in msg, msg
        assert (keep[0] == before).all()
        with pytest.raises(ValueError, match="16"):
            mcq_amd._lib.temper_counters_device(block(), type("S", (), {"cuda_stream": None})())
    block, keep = _block_maker(N=16)  # N = 16 itself is not what is refused
    assert L.mcq_temper_counters_device(ctypes.byref(block(n_chains=0)), None) == abi.EINVAL and b"n_chains" in L.mcq_temper_last_error()


def test_the_entry_point_refuses_what_mcq_temper_device_refuses_with_the_same_words():
    L = mcq_amd._lib.lib()
    block, keep = _block_maker()
    hist, rhist = np.zeros((8, 4), dtype=np.int32), np.zeros((8, 4), dtype=np.uint8)
    big = (1 << 63) // 36
    refused = ((dict(mode=abi.MODE_FULL3D), b"boards only"), (dict(N=1), b"N out of range"), (dict(N=129), b"N out of range"),
               (dict(n_chains=0), b"n_chains"), (dict(n_chains=1 << 31), b"n_chains"), (dict(replicas=3), b"2, 4, 8 or 16"),
               (dict(replicas=1), b"2, 4, 8 or 16"), (dict(replicas=32), b"2, 4, 8 or 16"), (dict(replicas=0), b"2, 4, 8 or 16"),
               (dict(replicas=16), b"must divide"), (dict(n_chains=6), b"must divide"), (dict(n_sweeps=-1), b"n_sweeps"),
               (dict(first_sweep=-1), b"first_sweep"), (dict(first_sweep=big), b"below 2^63"), (dict(exchange_every=0), b"exchange_every"),
               (dict(exchange_every=-2), b"exchange_every"), (dict(n_events=1), b"n_events"), (dict(n_events=3), b"n_events"),
               (dict(n_events=0), b"n_events"), (dict(exchange_every=1), b"n_events"), (dict(table_len=0), b"table_len"), (dict(table_len=513), b"table_len"),
               (dict(swap_len=0), b"swap_len"), (dict(swap_len=4097), b"swap_len"), (dict(seeds=None), b"seeds"), (dict(table=None), b"table is required"),
               (dict(swap_table=None), b"swap_table"), (dict(state_in=None), b"state_in"), (dict(state_out=None), b"state_out"),
               (dict(energy_hist=hist.ctypes.data, hist_stride=3), b"hist_stride"), (dict(rung_hist=rhist.ctypes.data, hist_stride=0), b"hist_stride"))
    for kw, msg in refused:
        assert L.mcq_temper_device(ctypes.byref(block(**kw)), None) == abi.EINVAL, kw
        lines = bytes(L.mcq_temper_last_error())
        assert msg in lines, (kw, lines)
        assert L.mcq_temper_host(ctypes.byref(block(n_sweeps=0, n_events=0))) == abi.OK  # (a good call in between leaves the message alone or not: it is set again below)
        assert L.mcq_temper_counters_device(ctypes.byref(block(**kw)), None) == abi.EINVAL, kw
        assert bytes(L.mcq_temper_last_error()) == lines, (kw, L.mcq_temper_last_error())
    assert L.mcq_temper_counters_device(None, None) == abi.EINVAL and b"NULL parameter block" in L.mcq_temper_last_error()
    # N = 2: 2^61 events times 16 replicas would wrap the exchange stream's word index
    wide = np.zeros((16, 4), dtype=np.uint8)
    q = block(N=2, n_chains=16, replicas=16, first_sweep=(1 << 61) - 8, n_sweeps=0, exchange_every=1, n_events=0, state_in=wide.ctypes.data, state_out=wide.ctypes.data)
    assert L.mcq_temper_counters_device(ctypes.byref(q), None) == abi.EINVAL and b"exchange stream" in L.mcq_temper_last_error()
    # an N the form does not run is refused for what the block gets wrong first, as mcq_temper_device would
    assert L.mcq_temper_counters_device(ctypes.byref(block(N=17, replicas=3)), None) == abi.EINVAL and b"2, 4, 8 or 16" in L.mcq_temper_last_error()


def test_python_refuses_before_any_gpu_call():
    """None of these reaches the GPU: there is none here."""
    boards, seeds = qu.random_boards(6, 64, 1), abi.seeds_for(42, 64)
    big = np.zeros((4, 17 * 17), dtype=np.uint8)
    ladder = [0.5, 1.0, 1.5, 2.0]
    with pytest.raises(ValueError, match="Unknown form"):
        tempering.temper_device(6, boards, seeds, [1.0], ladder, form="bytes")
    with pytest.raises(ValueError, match="Unknown form"):
        tempering.temper_states(6, boards, seeds, [1.0], ladder, form="auto")
    with pytest.raises(ValueError, match="Unknown form"):
        tempering.anneal_tempered(6, 10, boards, LIN, seeds, ladder, form="Lines")
    with pytest.raises(ValueError, match="N <= 16"):
        tempering.temper_device(17, big, [1, 2, 3, 4], [1.0], ladder, form="counters")
    with pytest.raises(ValueError, match="N <= 16"):
        tempering.temper_states(17, big, [1, 2, 3, 4], [1.0], ladder, form="counters")
    with pytest.raises(ValueError, match="N <= 16"):
        tempering.anneal_tempered(17, 10, "random", LIN, seeds, ladder, form="counters")
    with pytest.raises(ValueError, match='one form "lines"'):
        tempering.anneal_tempered(6, 10, "random", LIN, seeds, ladder, mcmc_type="full_3d", form="counters")
    with pytest.raises(ValueError, match="Unknown form"):
        tempering.anneal_tempered(6, 10, "random", LIN, seeds, ladder, mcmc_type="full_3d", form="bytes")
    # before anything else is looked at: a ladder that would be refused is not reached
    with pytest.raises(ValueError, match="Unknown form"):
        tempering.temper_states(6, boards, seeds, [1.0], [2.0, 1.0], form="bytes")
    with pytest.raises(ValueError, match="N <= 16"):
        tempering.anneal_tempered(17, 10, "random", [LIN, LIN], seeds[:5], ladder[::-1], form="counters")
    # the refusals that were there stay in front of nothing new: a good form goes on to them
    with pytest.raises(ValueError, match="one schedule"):
        tempering.anneal_tempered(6, 10, boards, [LIN, LIN], seeds, ladder, form="counters")
    with pytest.raises(ValueError, match="non-decreasing"):
        tempering.temper_states(6, boards, seeds, [1.0], [2.0, 1.0], form="counters")
    with pytest.raises(ValueError, match="contiguous uint8 tensor on the GPU"):
        tempering.temper_device(6, boards, seeds, [1.0], ladder, form="counters")


def test_a_form_reaches_its_entry_point(monkeypatch):
    """temper_device up to the library call with everything behind the form check stubbed: nothing is launched."""
    seen = []
    monkeypatch.setattr(mcq_amd._lib, "temper_device", lambda q, st: seen.append("lines"))
    monkeypatch.setattr(mcq_amd._lib, "temper_counters_device", lambda q, st: seen.append("counters"))
    monkeypatch.setattr(tempering, "_device_states", lambda name, N, states: 8)
    monkeypatch.setattr(tempering, "_device_call", lambda n, block, run, *a: run(block(3, 4, 5, 6), None))
    for form, want in ((None, "lines"), ("lines", "lines"), ("counters", "counters")):
        del seen[:]
        tempering.temper_device(6, object(), [0] * 8, [1.0] * 3, [0.5, 1.0, 1.5, 2.0], **({} if form is None else {"form": form}))
        assert seen == [want], (form, seen)
    # temper_states and anneal_tempered hand their form to temper_device
    import inspect

    for fn in (tempering.temper_states, tempering.anneal_tempered):
        assert "form=form" in inspect.getsource(fn), fn.__name__
