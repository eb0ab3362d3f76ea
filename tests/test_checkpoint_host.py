"""CPU-only: the host half of checkpoint / resume -- Checkpoint.merge against the reference's own histories cut in two, save / load, the
beta slices of a segment, the refusals of mcq_validate_resume, and the ABI's new names."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

import mcq_amd
from mcq_amd.checkpoint import Checkpoint

abi = mcq_amd.abi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIN = {"type": "linear_annealing", "beta_start": 1.0, "beta_end": 3.0}


def _segment(hist, acc):
    """What a call that ran this slice of a chain reports: hist has one entry more than acc."""
    return {"initial_energy": np.array([hist[0]]), "final_energy": np.array([hist[-1]]), "best_energy": np.array([hist.min()]),
            "steps_to_best": np.array([int(np.argmin(hist))]), "n_accepted": np.array([int(acc.sum())])}


def _merged(hist, acc, K, seed=0, N=6, mode="board"):
    c = Checkpoint(N, mode, len(hist) - 1, [seed], schedule_params=LIN)
    c.merge(_segment(hist[: K + 1], acc[:K]), K)
    c.merge(_segment(hist[K:], acc[K:]), len(hist) - 1 - K)
    return c


def test_merge_of_two_halves_is_the_whole_chain(golden):
    cases = [c for c in golden.chains if c.get("patience") is None and c["n_steps"] >= 200]
    cases = [c for c in cases if c["mode"] == "board"][:14] + [c for c in cases if c["mode"] == "full_3d"][:14]
    assert len(cases) >= 20
    for case in cases:
        g = golden.chain(case)
        n = case["n_steps"]
        hist = np.asarray(g["hist"], dtype=np.int64)
        acc = np.unpackbits(np.asarray(g["accept"], dtype=np.uint8), bitorder="little")[:n]
        assert len(hist) == n + 1
        for K in (1, 15, 16, 17, 63, 64, 65, n // 2, n - 1):
            c = _merged(hist, acc, K, seed=case["seed"], N=case["N"], mode=case["mode"])
            what = f"{case} cut at {K}"
            assert int(c.best_energy[0]) == int(g["best_energy"]), what
            assert int(c.steps_to_best[0]) == int(g["steps_to_best"]), what
            assert int(c.energy[0]) == int(g["final_energy"]), what
            assert int(c.n_accepted[0]) == int(acc.sum()) and c.step == n, what
    # a chain whose minimum occurs in both halves: the first index stays
    hist, acc = np.array([5, 3, 4, 3, 6]), np.array([1, 1, 1, 1])
    c = _merged(hist, acc, 2)
    assert (int(c.best_energy[0]), int(c.steps_to_best[0]), int(c.energy[0]), int(c.n_accepted[0])) == (3, 1, 6, 4)
    c = _merged(np.array([5, 4, 4, 3, 6]), acc, 2)  # ... and a strictly lower one in the second half moves it
    assert (int(c.best_energy[0]), int(c.steps_to_best[0])) == (3, 3)


def test_merge_follows_the_best_state_and_checks_the_seam():
    c = Checkpoint(2, "board", 10, [1, 2], schedule_params=LIN)
    s1 = {"initial_energy": np.array([9, 9]), "final_energy": np.array([7, 8]), "best_energy": np.array([6, 8]), "steps_to_best": np.array([2, 4]),
          "n_accepted": np.array([3, 1]), "stream_words": np.array([40, 44], dtype=np.uint32), "best_state": np.array([[1, 1, 1, 1], [2, 2, 2, 2]], dtype=np.uint8),
          "final_state": np.zeros((2, 4), dtype=np.uint8), "stream_state": np.zeros((2, 625), dtype=np.uint32)}
    c.merge(s1, 5)
    s2 = dict(s1, initial_energy=np.array([7, 8]), final_energy=np.array([6, 5]), best_energy=np.array([6, 5]), steps_to_best=np.array([5, 3]),
              stream_words=np.array([0xFFFFFFF0, 30], dtype=np.uint32), best_state=np.array([[3, 3, 3, 3], [0, 1, 0, 1]], dtype=np.uint8))
    c.merge(s2, 5)
    assert c.best_energy.tolist() == [6, 5] and c.steps_to_best.tolist() == [2, 8] and c.n_accepted.tolist() == [6, 2] and c.step == 10
    assert c.best_state.tolist() == [[1, 1, 1, 1], [0, 1, 0, 1]]
    assert c.stream_words.dtype == np.uint64 and c.stream_words.tolist() == [40 + 0xFFFFFFF0, 74]  # a running 64-bit total
    with pytest.raises(ValueError, match="leaves the schedule"):
        c.merge(s2, 1)
    c = Checkpoint(2, "board", 10, [1, 2], schedule_params=LIN).merge(s1, 5)
    with pytest.raises(ValueError, match="chain 1: the segment starts at energy 9"):
        c.merge(dict(s2, initial_energy=np.array([7, 9])), 5)


def test_save_load_round_trip_and_refusals(tmp_path):
    sets = [LIN, {"type": "constant", "beta_const": 2.0}]
    c = Checkpoint(5, "full_3d", 100, np.arange(32), schedule_sets=sets, chains_per_set=16, trace="reduced")
    rs = np.random.RandomState(1)
    seg = {"initial_energy": rs.randint(0, 50, 32), "final_energy": rs.randint(0, 50, 32), "best_energy": rs.randint(0, 9, 32), "steps_to_best": rs.randint(0, 40, 32),
           "n_accepted": rs.randint(0, 40, 32), "stream_words": rs.randint(0, 2**32, 32, dtype=np.uint32), "best_state": rs.randint(0, 5, (32, 75)).astype(np.uint8),
           "final_state": rs.randint(0, 5, (32, 75)).astype(np.uint8), "stream_state": rs.randint(0, 2**32, (32, 625), dtype=np.uint32)}
    c.merge(seg, 40)
    path = str(tmp_path / "c.npz")
    c.save(path)
    with np.load(path, allow_pickle=False) as z:  # plain arrays only
        assert "meta" in z.files and z["stream_state"].dtype == np.uint32
    d = Checkpoint.load(path)
    assert (d.N, d.mode, d.Q, d.schedule_steps, d.step, d.trace, d.chains_per_set) == (5, "full_3d", 25, 100, 40, "reduced", 16)
    assert d.schedule_sets == sets and d.schedule_params is None
    for k in ("seeds", "state", "stream_state", "energy", "best_energy", "best_state", "steps_to_best", "n_accepted", "stream_words"):
        a, b = getattr(c, k), getattr(d, k)
        assert a.dtype == b.dtype and np.array_equal(a, b), k
    d.require(N=5, mcmc_type="full_3d", Q=25)
    for kw, msg in ((dict(N=6), "N = 5"), (dict(mcmc_type="board"), "full_3d chains"), (dict(Q=20), "Q = 25")):
        with pytest.raises(ValueError, match=msg):
            d.require(**kw)
        with pytest.raises(ValueError, match=msg):  # continue_chains refuses before anything is launched
            mcq_amd.experiments.continue_chains(d, 10, **kw)
    with pytest.raises(ValueError, match="one schedule"):
        Checkpoint(5, "board", 10, [1])


def test_beta_of_a_segment_is_a_slice_of_the_whole_table(golden):
    z = golden.npz("beta")
    for c in golden.manifest["beta"]:
        total = c["n_steps"]
        if total < 1000:
            continue
        whole = abi.beta_values(c["schedule"], total)
        np.testing.assert_array_equal(whole[z[c["key"] + "_steps"]], z[c["key"] + "_beta"], err_msg=str(c))  # the reference's own values
        for first, n in ((0, 1), (0, 17), (1, 63), (total // 2, 100), (total - 1, 1), (total - 64, 64)):
            p = abi.make_params(6, n, "random", c["schedule"], 2, mcmc_type="board")
            tab = abi.segment_beta_table(p, first, total)
            assert tab.shape == (1, n) and tab.dtype == np.float64
            assert tab.tobytes() == whole[first: first + n].tobytes(), (c, first, n)
    types = {c["schedule"]["type"] for c in golden.manifest["beta"] if c["n_steps"] >= 1000}
    assert types == set(abi.SCHED)
    sets = [{"type": "sinusoidal_annealing", "beta_start": 0.1, "beta_end": 2.0}, {"type": "exponential_annealing", "beta_start": 1.0, "beta_end": 3.0}]
    p = abi.make_params_sets(6, 50, "random", sets, 16, mcmc_type="board")
    tab = abi.segment_beta_table(p, 30, 500)
    for t in range(2):
        assert tab[t].tobytes() == abi.beta_values(sets[t], 500)[30:80].tobytes()


def _refused(p, r):
    L = mcq_amd._lib.lib()
    rc = L.mcq_validate_resume(ctypes.byref(p), ctypes.byref(r))
    return rc, L.mcq_last_error().decode()


def test_validate_resume_refuses_what_is_not_built():
    make = abi.make_params
    p = make(6, 100, "random", LIN, 16, mcmc_type="board")
    assert _refused(p, abi.make_resume(p, 0, 100))[0] == abi.OK
    assert _refused(p, abi.make_resume(p, 900, 1000))[0] == abi.OK
    state, stream = np.zeros((16, 36), dtype=np.uint8), np.zeros((16, 625), dtype=np.uint32)
    assert _refused(p, abi.make_resume(p, 10, 200, state=state, stream_state=stream))[0] == abi.OK
    for first, total in ((-1, 1000), (901, 1000), (0, 99)):
        rc, msg = _refused(p, abi.make_resume(p, first, total))
        assert rc == abi.EINVAL and ("first_step" in msg), (first, total, msg)
    # Philox with a stream or a state
    q = make(6, 100, "random", LIN, 16, mcmc_type="board", rng="philox")
    rc, msg = _refused(q, abi.make_resume(q, 0, 100, state=state, stream_state=stream))
    assert rc == abi.EINVAL and "Philox" in msg
    rc, msg = _refused(q, abi.make_resume(q, 0, 100, state=state))
    assert rc == abi.EINVAL and "Philox" in msg
    # replica exchange
    q = abi.set_exchange(make(6, 100, "random", LIN, 16, mcmc_type="board"), 10, [1.0, 0.8])
    rc, msg = _refused(q, abi.make_resume(q, 0, 100))
    assert rc == abi.EINVAL and "replica exchange" in msg
    # early stopping that could trigger: 0 <= patience <= schedule_steps (a board; full_3d ignores the patience)
    for patience, total, ok in ((0, 100, False), (100, 100, False), (150, 1000, False), (1001, 1000, True), (None, 1000, True)):
        q = make(6, 100, "random", LIN, 16, mcmc_type="board", early_stop_patience=patience)
        rc, msg = _refused(q, abi.make_resume(q, 0, total))
        assert (rc == abi.OK) == ok and (ok or "early stopping" in msg), (patience, total, msg)
    q = make(6, 100, "random", LIN, 16, mcmc_type="full_3d", early_stop_patience=5)
    assert _refused(q, abi.make_resume(q, 0, 100))[0] == abi.OK
    # a stream without a state, a state next to stream_states, a misaligned state
    rc, msg = _refused(p, abi.make_resume(p, 0, 100, stream_state=stream))
    assert rc == abi.EINVAL and "stream without state" in msg
    q = abi.set_stream_states(make(6, 100, "random", LIN, 16, mcmc_type="board"), np.zeros((16, 625), dtype=np.uint32))
    assert _refused(q, abi.make_resume(q, 0, 100))[0] == abi.OK  # a first segment may continue a caller's stream
    rc, msg = _refused(q, abi.make_resume(q, 0, 100, state=state))
    assert rc == abi.EINVAL and "stream_states" in msg
    r = abi.make_resume(p, 0, 100, state=state)
    r.state += 4
    rc, msg = _refused(p, r)
    assert rc == abi.EINVAL and "aligned" in msg
    # through the Python wrapper: ValueError
    with pytest.raises(ValueError, match="first_step"):
        mcq_amd._lib.validate_resume(p, abi.make_resume(p, 5, 100))
    with pytest.raises(ValueError, match="must be uint8"):
        abi.make_resume(p, 0, 100, state=np.zeros((16, 35), dtype=np.uint8))
    # run_experiment names the way past the row limit, and refuses a segment length that has the same problem
    with pytest.raises(ValueError, match="segment_steps"):
        mcq_amd.experiments.run_experiment(6, 100, "random", None, 2, schedule_params=LIN, mcmc_type="board", early_stop_patience=None, segment_steps=1 << 24)


def test_checkpoint_refuses_philox_and_overlong_segments():
    """mcq_checkpoint_device's own MCQ_EINVAL (include/mcq.h), decided before anything touches a device."""
    L = mcq_amd._lib.lib()
    out = abi.Outputs()
    dummy = ctypes.c_void_p(4096)  # never dereferenced: the parameters are refused first
    for kw, n_steps, msg in ((dict(rng="philox"), 100, "Philox"), ({}, (1 << 28) + 1, "2\\^28 steps")):
        p = abi.make_params(6, n_steps, "random", LIN, 16, mcmc_type="board", trace=False, **kw)
        rc = L.mcq_checkpoint_device(ctypes.byref(p), ctypes.byref(out), dummy, ctypes.c_size_t(1 << 40), dummy, None)
        assert rc == abi.EINVAL and __import__("re").search(msg, L.mcq_last_error().decode()), (kw, n_steps, L.mcq_last_error())
    p = abi.make_params(6, 100, "random", LIN, 16, mcmc_type="board")
    assert L.mcq_checkpoint_device(ctypes.byref(p), ctypes.byref(out), None, ctypes.c_size_t(1 << 40), dummy, None) == abi.EINVAL


def test_new_symbols_and_the_resume_mirror():
    L = mcq_amd._lib.lib()
    for n in ("mcq_validate_resume", "mcq_run_device_from", "mcq_run_device_from_timed", "mcq_checkpoint_device", "mcq_run_host_from"):
        assert hasattr(L, n), n
    assert L.mcq_abi_version() == abi.ABI_VERSION == 6
    fields = [f for f, _ in abi.Resume._fields_]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "mcq.h"\nint main(){printf("%zu", sizeof(mcq_resume));' + \
        "".join(f'printf(" %zu", offsetof(mcq_resume, {f}));' for f in fields) + "return 0;}"
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(prog)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")], check=True)
        out = subprocess.run([os.path.join(d, "t")], capture_output=True, text=True, check=True).stdout.split()
    assert int(out[0]) == ctypes.sizeof(abi.Resume)
    assert [int(x) for x in out[1:]] == [getattr(abi.Resume, f).offset for f in fields]
    # the parameter and output blocks kept their layout: the workspace of a run is what it was
    p = abi.make_params(12, 1000, "random", {"type": "constant", "beta_const": 1.0}, 10, mcmc_type="board")
    assert L.mcq_workspace_bytes(ctypes.byref(p)) == 8192 + 4096 + 2048 * 16 * 4 + 128 + 10 * 672 * 4


def test_the_build_sees_the_second_source_and_the_shared_header():
    b = mcq_amd.build
    names = {os.path.basename(f) for f in b.SOURCES + b.HEADERS}
    assert {"mcq_hip.hip", "mcq_resume.hip", "mcq_record.h", "mcq.h"} <= names
    assert all(os.path.exists(f) for f in b.SOURCES + b.HEADERS)
