"""GPU: the counter form of the heat-bath column sweep (mcq_heatbath_counters_device, form="counters") against the library's host code
(mcq_heatbath_host) and against the lines form (mcq_heatbath_device) bit for bit on every output, for every N it runs; its energies
against the quench kernel's recount after many changed heights; ragged chain counts; segments; the edge cases of the weight table;
anneal_heatbath and the competition driver with either form; torch tensors on a stream of its own; and the refusal of N = 17."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import mcq_amd
from tests import heatbath_counters_util as cu
from tests import heatbath_util as hu
from tests import population_util as pu
from tests import quench_util as qu
from tests.heatbath_tables_util import host_with_table as _host_with_table

abi = mcq_amd.abi
heatbath = mcq_amd.heatbath
quench = mcq_amd.quench
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIN = {"type": "linear_annealing", "beta_start": 1.0, "beta_end": 3.0}

# beta = 0 changes about (N - 1) / N of the heights: the most counter updates there can be; [] is a recount and a copy
BETAS = ((0.0, 3.0, 1.0), (0.5, 0.5), (3.0,), (0.004,), [50.0], [])


def _boards(N, n, seed):
    """tests/test_heatbath.py's boards (random, one all-equal, one all-255), and where there is room h = (i + j) mod N and h = i, which
    fill whole diagonal lines: the largest counter there can be, N."""
    s = qu.random_boards(N, n, seed, over=seed % 2 == 1)
    s[0] = seed % N  # all heights equal
    if n > 2:
        s[1] = 255  # clamped
        s[2] = cu.special_boards(N)[0]
    if n > 3:
        s[3] = cu.special_boards(N)[1]
    return s


def _seeds(n, k):
    s = (np.arange(n, dtype=np.uint64) * 2654435761 + k) % 2**32
    s[-1] = 2**32 - 1
    return s.astype(np.uint32)


@pytest.mark.parametrize("N", range(2, 17))
def test_kernel_equals_the_host_code_and_the_lines_kernel(N):
    firsts = (0, 3, (1 << 34) // (N * N) + 5, 1 << 40)
    m = 0
    for idx, n in enumerate((1, 3, 5, 17)):
        for t, betas in enumerate(BETAS):
            first, trace = firsts[m % 4], (m // 4) % 2 == 0  # over the 24 cases: every first_sweep with the trace on and off
            m += 1
            s, seeds = _boards(N, n, 100 * N + idx), _seeds(n, N + t)
            what = f"N={N}, {n} chains, betas={betas}, first_sweep={first}"
            want = heatbath.heatbath_states_host(N, s, seeds, betas, first_sweep=first, trace=trace)
            got = heatbath.heatbath_states(N, s, seeds, betas, first_sweep=first, trace=trace, form="counters")
            hu.assert_equal(got, want, what + ": counters vs the host code", hist=trace)
            assert set(got) == set(want)
            for k in want:
                assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
            lines = heatbath.heatbath_states(N, s, seeds, betas, first_sweep=first, trace=trace, form="lines")
            hu.assert_equal(got, lines, what + ": counters vs lines", hist=trace)
    # against the restatement too
    s, seeds = _boards(N, 4, 7 * N), _seeds(4, 1)
    hu.assert_equal(heatbath.heatbath_states(N, s, seeds, (0.0, 3.0), first_sweep=2, trace=True, form="counters"), hu.sweeps_many(N, s, seeds, (0.0, 3.0), 2),
                    f"N={N} vs the restatement", hist=True)


@pytest.mark.parametrize("N", (5, 12, 16))
def test_no_drift_after_many_changed_heights(N):
    n, betas = 9, [0.0] * 40 + [3.0] * 10
    s, seeds = _boards(N, n, 11 * N), _seeds(n, 5)
    got = heatbath.heatbath_states(N, s, seeds, betas, trace=True, form="counters")
    np.testing.assert_array_equal(quench.quench_states(N, got["state"])["energy_in"], got["energy_out"], err_msg="the quench kernel's recount of state")
    np.testing.assert_array_equal(got["energy_hist"][:, -1], got["energy_out"])
    want = heatbath.heatbath_states_host(N, s, seeds, betas, trace=True)
    np.testing.assert_array_equal(got["n_changed"], want["n_changed"])
    assert (got["n_changed"] > 40 * N * N * (N - 1) // N * 0.9).all()  # beta = 0: about (N - 1) / N of 40 N^2 updates changed a height
    hu.assert_equal(got, want, f"N={N}, 50 sweeps", hist=True)


def test_ragged_chain_counts_around_the_wavefront():
    for N, counts in ((12, (2, 4, 6, 7, 63, 64, 65, 1025)), (8, (255, 257))):
        for n in counts:
            s, seeds = _boards(N, n, N + n), _seeds(n, n)
            betas = (0.3, 2.5)
            want = heatbath.heatbath_states_host(N, s, seeds, betas, first_sweep=n, trace=True)
            got = heatbath.heatbath_states(N, s, seeds, betas, first_sweep=n, trace=True, form="counters")
            hu.assert_equal(got, want, f"N={N}, {n} chains", hist=True)


def test_more_workgroups_than_one_round_of_the_device():
    N, n, betas = 12, 4099, (0.0, 1.0, 2.0, 3.0)
    s, seeds = _boards(N, n, 3), abi.seeds_for(42, n)
    got = heatbath.heatbath_states(N, s, seeds, betas, first_sweep=1, trace=True, form="counters")
    lines = heatbath.heatbath_states(N, s, seeds, betas, first_sweep=1, trace=True, form="lines")
    hu.assert_equal(got, lines, "4 099 chains, counters vs lines", hist=True)
    assert got["n_changed"].sum() > 0 and (got["energy_out"] != got["energy_in"]).any()


def test_segments_in_place_equal_the_unbroken_call():
    import torch

    N, n, first = 13, 7, (1 << 35) // 169
    dev = torch.device("cuda", torch.cuda.current_device())
    st = torch.cuda.current_stream(dev)
    betas = np.array([0.0, 0.5, 1.0, 2.0, 3.0])
    s, seeds = _boards(N, n, 31 * N), _seeds(n, 3)
    whole = heatbath.heatbath_states(N, s, seeds, betas, first_sweep=first, trace=True, form="counters")
    hu.assert_equal(whole, heatbath.heatbath_states_host(N, s, seeds, betas, first_sweep=first, trace=True), "N=13, 5 sweeps", hist=True)
    t = torch.from_numpy(s).to(dev)
    a = heatbath.heatbath_device(N, t, seeds, betas[:2], first_sweep=first, out=t, trace=True, form="counters")
    assert a["state"] is t
    st.synchronize()
    ha = a["energy_hist"].cpu().numpy()
    b = heatbath.heatbath_device(N, t, seeds, betas[2:], first_sweep=first + 2, out=t, trace=True, form="counters")
    st.synchronize()
    hb = b["energy_hist"].cpu().numpy()
    np.testing.assert_array_equal(t.cpu().numpy(), whole["state"])
    np.testing.assert_array_equal(hb[:, 0], ha[:, -1], err_msg="the recount at the cut")
    np.testing.assert_array_equal(np.concatenate([ha, hb[:, 1:]], axis=1), whole["energy_hist"])
    np.testing.assert_array_equal(b["energy_out"].cpu().numpy(), whole["energy_out"])
    np.testing.assert_array_equal((a["n_changed"] + b["n_changed"]).cpu().numpy(), whole["n_changed"])


def test_a_table_of_one_entry_makes_every_update_uniform():
    """D = 1: every height has the weight T[0], so k = floor(x N / 2^32) whatever the placement."""
    import torch

    dev = torch.device("cuda", torch.cuda.current_device())
    for N in (2, 9, 16):
        Q, first = N * N, 3
        seeds = np.array([17, 4000000000], dtype=np.uint32)
        tab = np.full((2, 1), 1 << 24, dtype=np.uint32)
        dtab = torch.from_numpy(tab.view(np.int32)).to(dev)
        outs = []
        for boards in (qu.random_boards(N, 2, N, over=True), np.zeros((2, Q), dtype=np.uint8)):
            res = heatbath.heatbath_device(N, torch.from_numpy(boards).to(dev), seeds, dtab, first_sweep=first, trace=True, form="counters")
            torch.cuda.current_stream(dev).synchronize()
            got = heatbath.to_numpy(res)
            hu.assert_equal(got, _host_with_table(N, boards, seeds, tab, first, True), f"N={N}, D = 1", hist=True)
            outs.append(got["state"])
        np.testing.assert_array_equal(outs[0], outs[1], err_msg=f"N={N}: the placement mattered")
        for r in range(2):
            want = [(hu.word(int(seeds[r]), (first + 1) * Q + c) * N) >> 32 for c in range(Q)]  # the second sweep's words are what is left
            assert [int(v) for v in outs[0][r]] == want, (N, r)


def test_a_table_with_a_zero_never_raises_the_energy():
    """T = [2^24, 0]: only the heights of the smallest count have a weight."""
    import torch

    N, n, n_sweeps = 9, 6, 5
    dev = torch.device("cuda", torch.cuda.current_device())
    tab = np.tile(np.array([[1 << 24, 0]], dtype=np.uint32), (n_sweeps, 1))
    dtab = torch.from_numpy(tab.view(np.int32)).to(dev)
    s, seeds = _boards(N, n, 8), _seeds(n, 2)
    res = {}
    for form in heatbath.FORMS:
        r = heatbath.heatbath_device(N, torch.from_numpy(s).to(dev), seeds, dtab, first_sweep=1, trace=True, form=form)
        torch.cuda.current_stream(dev).synchronize()
        res[form] = heatbath.to_numpy(r)
    want = _host_with_table(N, s, seeds, tab, 1, True)
    hu.assert_equal(res["counters"], want, "T = [2^24, 0] vs the host code", hist=True)
    hu.assert_equal(res["counters"], res["lines"], "T = [2^24, 0] vs lines", hist=True)
    hist = res["counters"]["energy_hist"]
    assert (np.diff(hist, axis=1) <= 0).all() and (hist[:, -1] < hist[:, 0]).any()
    np.testing.assert_array_equal(res["counters"]["best_energy"], hist[:, -1])


@pytest.mark.parametrize("kw", (dict(), dict(resample_every=3, population=32, resample_seed=2), dict(quench=True)), ids=("plain", "resampled", "quench"))
def test_anneal_heatbath_with_counters_equals_lines(kw):
    N, n, n_sweeps = 6, 64, 12
    seeds, start = abi.seeds_for(42, n), qu.random_boards(6, n, 30)
    runs = {form: heatbath.anneal_heatbath(N, n_sweeps, start, LIN, seeds, trace=True, form=form, **kw) for form in heatbath.FORMS}
    a, b = runs["counters"], runs["lines"]
    if "resample_every" in kw:
        (a, la), (b, lb) = a, b
        assert set(la) == set(lb) and set(pu.LINEAGE_FIELDS) <= set(la)
        for k in lb:
            np.testing.assert_array_equal(np.asarray(la[k]), np.asarray(lb[k]), err_msg=f"lineage {k}")
        assert (la["distinct_parents"] < la["population"]).any(), "no boundary resampled anything"
    assert set(a) == set(b) and ("quenched_energy" in a) == bool(kw.get("quench"))
    for k in b:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    assert a["n_changed"].sum() > 0


def test_the_competition_driver_forwards_the_form(tmp_path, monkeypatch):
    drv = mcq_amd.drivers.run_competition
    seen = []
    real = heatbath.heatbath_device
    monkeypatch.setattr(heatbath, "heatbath_device", lambda *a, **k: (seen.append(k.get("form")), real(*a, **k))[1])
    e1, h1, p1 = drv(N=12, n_runs=32, n_steps=7, out_dir=str(tmp_path), timestamp="c", heatbath_sweeps=10, heatbath_form="counters")
    assert seen and set(seen) == {"counters"}
    del seen[:]
    e2, h2, p2 = drv(N=12, n_runs=32, n_steps=7, out_dir=str(tmp_path), timestamp="l", heatbath_sweeps=10)
    assert seen and set(seen) == {"lines"}
    assert e1 == e2 and os.path.exists(p1) and os.path.exists(p2)
    np.testing.assert_array_equal(h1, h2)


def test_torch_tensors_on_a_side_stream_in_a_fresh_process(tmp_path):
    """heatbath_device(form="counters") on a non-default stream with no synchronise inside: the call returns while a long kernel queued
    before it on the same stream still holds the stream, and the results are right once the stream is waited for."""
    out = str(tmp_path / "h.npz")
    code = f"""
import sys, numpy as np
sys.path.insert(0, {ROOT!r})
import torch, mcq_amd
from tests import quench_util as qu
dev = torch.device("cuda", 0)
s = qu.random_boards(12, 4099, 77, over=True)
seeds = mcq_amd.abi.seeds_for(9, 4099)
betas = [0.0, 2.0, 3.0]
side = torch.cuda.Stream(dev)
t = torch.from_numpy(s).to(dev)
dseeds = torch.from_numpy(seeds.view(np.int32)).to(dev)
dtab = mcq_amd.heatbath.device_table(betas, dev)
mcq_amd.heatbath.heatbath_device(12, t[:8].contiguous(), seeds[:8], betas, form="counters")  # the first launch loads the library's code object: not part of what is shown
torch.cuda.synchronize()
syncs = []
real = torch.cuda.Stream.synchronize
torch.cuda.Stream.synchronize = lambda self: (syncs.append("stream"), real(self))[1]
real_all = torch.cuda.synchronize
torch.cuda.synchronize = lambda *a, **k: (syncs.append("device"), real_all(*a, **k))[1]
with torch.cuda.stream(side):
    big = torch.empty(1 << 28, dtype=torch.float32, device=dev)
    for _ in range(50):
        big.add_(1.0)  # ~ tens of milliseconds of work ahead of the sweeps on the side stream
    res = mcq_amd.heatbath.heatbath_device(12, t, dseeds, dtab, first_sweep=3, trace=True, form="counters")  # (stream=None: torch's current stream, which is `side`)
    pending = not side.query()
torch.cuda.Stream.synchronize, torch.cuda.synchronize = real, real_all
side.synchronize()
got = mcq_amd.heatbath.to_numpy(res)
np.savez({out!r}, pending=pending, n_syncs=len(syncs), inp=s, seeds=seeds, **got)
"""
    done = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-c", code], cwd=ROOT)
    assert done.returncode == 0, f"the child process ended with status {done.returncode}"
    with np.load(out) as z:
        assert int(z["n_syncs"]) == 0, "heatbath_device synchronised"
        assert bool(z["pending"]), "the stream had drained before heatbath_device returned: the call cannot be shown to be asynchronous"
        want = heatbath.heatbath_states_host(12, z["inp"], z["seeds"], [0.0, 2.0, 3.0], first_sweep=3, trace=True)
        hu.assert_equal({k: z[k] for k in hu.FIELDS + ("energy_hist",)}, want, "side stream, fresh process", hist=True)


def test_the_entry_point_refuses_n_17_and_launches_nothing():
    import torch

    N, n = 17, 3
    dev = torch.device("cuda", torch.cuda.current_device())
    st = torch.cuda.current_stream(dev)
    tab = torch.from_numpy(abi.heatbath_table([1.0]).view(np.int32)).to(dev)
    sd = torch.zeros(n, dtype=torch.int32, device=dev)
    t = torch.zeros((n, N * N), dtype=torch.uint8, device=dev)
    o = torch.full((n, N * N), 201, dtype=torch.uint8, device=dev)
    e = torch.full((n,), -77, dtype=torch.int32, device=dev)
    q = abi.Heatbath()
    q.N, q.mode, q.n_chains, q.n_sweeps, q.first_sweep, q.table_len = N, abi.MODE_BOARD, n, 1, 0, tab.shape[1]
    q.seeds, q.table, q.state_in, q.state_out, q.energy_out = sd.data_ptr(), tab.data_ptr(), t.data_ptr(), o.data_ptr(), e.data_ptr()
    L = mcq_amd._lib.lib()
    assert L.mcq_heatbath_counters_device(ctypes.byref(q), ctypes.c_void_p(st.cuda_stream)) == abi.EINVAL
    assert b"16" in L.mcq_heatbath_last_error(), L.mcq_heatbath_last_error()
    with pytest.raises(ValueError, match="16"):
        mcq_amd._lib.heatbath_counters_device(q, st)
    st.synchronize()
    assert (o.cpu().numpy() == 201).all() and (e.cpu().numpy() == -77).all(), "something was launched"
    mcq_amd._lib.heatbath_device(q, st)  # the lines form takes the same block
    st.synchronize()
    assert (o.cpu().numpy() < N).all() and (e.cpu().numpy() >= 0).all()
