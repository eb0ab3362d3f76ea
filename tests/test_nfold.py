"""GPU: the n-fold kernel (mcq_nfold_device) against the library's host code (mcq_nfold_host) bit for bit on every output and dtype at
both ends of every instantiation -- 67 chains, 5 segments of 40 Metropolis steps under rows from beta = 0 to beta = 8, both clocks, with
and without the history --; device segments with the need and the event counter carried on the device against the unbroken launch;
strict minima that sleep; the 4096 events of a step under a clock of zeros; N = 32 at beta = 0; an event counter that crosses 2^32; in
place; a side stream in a fresh process; anneal_nfold against the same run composed from the host code; and the refusals of N = 33 and
full_3d before any launch.  tests/test_nfold_host.py holds the host code to the NumPy restatement of the rule."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import mcq_amd
from tests import quench_util as qu

abi = mcq_amd.abi
nfold = mcq_amd.nfold
quench = mcq_amd.quench
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the instantiations are padded N = 4, 8, 12, 16, 24, 32: both ends of each
SIZES = (2, 4, 5, 8, 9, 12, 13, 16, 17, 24, 25, 32)
CHAINS, SEGS, STEPS = 67, 5, 40  # more than 64 workgroups
BETAS = (0.0, 0.3, 1.0, 3.0, 8.0)
INT_FIELDS = tuple(k for k in nfold.FIELDS if k != "energy_hist")


@functools.lru_cache(maxsize=None)
def _case(N, clock):
    """(placements with bytes >= N, seeds, rows, the host code's result with the history): computed once, shared and left unchanged."""
    s = qu.random_boards(N, CHAINS, 500 + N, over=True)
    seeds = abi.seeds_for(4000000000 + 100 * N, CHAINS)
    tabs = nfold.weight_tables(BETAS)
    return s, seeds, tabs, nfold.nfold_states_host(N, s, seeds, tabs, STEPS, clock=clock, hist=True)


def _assert_same(got, want, what, fields=nfold.FIELDS):
    for k in fields:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].dtype, want[k].dtype)
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{what}: {k}")


@pytest.mark.parametrize("clock", nfold.CLOCKS)
@pytest.mark.parametrize("N", SIZES)
def test_kernel_equals_the_host_code(N, clock):
    s, seeds, tabs, want = _case(N, clock)
    # what the comparison covers, from the host code's outputs: events in every chain, rises and flat moves, a best below the input
    assert (want["events_out"] > SEGS).all() and (N == 2 or (want["n_uphill"].sum() > 0 and want["n_flat"].sum() > 0))
    assert N == 2 or ((want["best_energy"] < want["energy_in"]).any() and (want["best_step"] > 0).any())
    got = nfold.nfold_states(N, s, seeds, tabs, STEPS, clock=clock, hist=True)
    _assert_same(got, want, f"N = {N}, {clock}")
    slim = nfold.nfold_states(N, s, seeds, tabs, STEPS, clock=clock)
    assert "energy_hist" not in slim
    _assert_same(slim, want, f"N = {N}, {clock}, no history", fields=INT_FIELDS)


@pytest.mark.parametrize("N", (5, 12, 17, 32))
def test_segments_carried_on_the_device_are_the_unbroken_launch(N):
    import torch

    dev = torch.device("cuda", torch.cuda.current_device())
    s, seeds, tabs, want = _case(N, "exp")
    t, sd = torch.from_numpy(s).to(dev), torch.from_numpy(seeds.view(np.int32)).to(dev)
    dtab = torch.from_numpy(tabs.view(np.int32)).to(dev)
    ln2, ct = nfold.clock_tables("exp")
    clock = (ln2, torch.from_numpy(ct.view(np.int32)).to(dev))
    state, need, events, pieces = t, None, None, []
    for first, last in ((0, 1), (1, 1), (1, 3), (3, 5)):  # a piece of no segment among them; nothing is copied back in between
        res = nfold.nfold_device(N, state, sd, dtab[first:last], STEPS, first_seg=first, clock=clock, need_in=need, events_in=events, hist=True)
        state, need, events = res["state"], res["need_out"], res["events_out"]
        pieces.append(res)
    torch.cuda.current_stream(dev).synchronize()
    out = [nfold.to_numpy(p) for p in pieces]
    for k in ("state", "energy_out", "events_out", "need_out", "weight_out"):
        np.testing.assert_array_equal(out[-1][k], want[k], err_msg=k)
    np.testing.assert_array_equal(np.concatenate([out[0]["energy_hist"]] + [o["energy_hist"][:, 1:] for o in out[1:]], axis=1), want["energy_hist"])
    np.testing.assert_array_equal(sum(o["n_uphill"] for o in out), want["n_uphill"])
    np.testing.assert_array_equal(sum(o["n_flat"] for o in out), want["n_flat"])
    best = np.minimum.reduce([o["best_energy"] for o in out])
    np.testing.assert_array_equal(best, want["best_energy"])
    starts = (0, 1, 1, 3)
    step = np.full(CHAINS, -1, dtype=np.int64)
    for o, first in reversed(list(zip(out, starts))):  # the first piece that holds the best
        step = np.where(o["best_energy"] == best, o["best_step"] + first * STEPS, step)
    np.testing.assert_array_equal(step, want["best_step"])
    np.testing.assert_array_equal(t.cpu().numpy(), s)  # out of place: the input is untouched


def test_strict_minima_sleep_on_the_device():
    N = 5
    q = quench.quench_pairs_host(N, qu.random_boards(N, 400, N), conflicts=False)["state"]
    row = np.array([[1 << 24, 0]], dtype=np.uint32)
    m = q[nfold.nfold_states_host(N, q, abi.seeds_for(1, len(q)), row, 1)["weight_out"] == 0]
    assert len(m) >= 3
    n = len(m)
    need = (np.arange(n, dtype=np.uint64) * 12345 + 1) << 20
    ev = np.arange(n, dtype=np.int64) + 2**33
    rows = np.repeat(row, 3, axis=0)
    want = nfold.nfold_states_host(N, m, abi.seeds_for(5, n), rows, 1 << 31, need_in=need, events_in=ev, hist=True)
    got = nfold.nfold_states(N, m, abi.seeds_for(5, n), rows, 1 << 31, need_in=need, events_in=ev, hist=True)
    _assert_same(got, want, "sleeping minima")
    np.testing.assert_array_equal(got["need_out"], need)
    np.testing.assert_array_equal(got["events_out"], ev)
    np.testing.assert_array_equal(got["state"], m)
    assert (got["weight_out"] == 0).all()


def test_a_clock_of_zeros_fires_4096_events_per_step_on_the_device():
    N, n, S = 3, 70, 2
    s = qu.random_boards(N, n, 12)
    seeds = abi.seeds_for(31, n)
    tabs = nfold.weight_tables([0.0] * S)
    zero = (0, np.zeros(256, dtype=np.uint32))
    got = nfold.nfold_states(N, s, seeds, tabs, 1, clock=zero, hist=True)
    assert (got["events_out"] == S << abi.NFOLD_TIME_BITS).all() and (got["need_out"] == 0).all()
    _assert_same(got, nfold.nfold_states_host(N, s, seeds, tabs, 1, clock=zero, hist=True), "a clock of zeros")


def test_the_largest_board_with_every_weight_at_its_bound():
    """N = 32 at beta = 0: every weight is 2^24, R(c) = 31 2^24, a lane's 16 columns sum beyond 32 bits, W = M 2^24 just below 2^39, and
    U takes the whole 128-bit product."""
    N, n = 32, 9
    s = qu.random_boards(N, n, 32)
    seeds = abi.seeds_for(4294967000, n)
    tabs = nfold.weight_tables([0.0, 0.0])
    want = nfold.nfold_states_host(N, s, seeds, tabs, 30, hist=True)
    assert (want["weight_out"] == N * N * (N - 1) << 24).all() and (want["events_out"] > 30).all()
    moved = (want["state"] != s).nonzero()[1]
    assert moved.min() < 64 and moved.max() >= N * N - 64  # the draw reaches the first and the last lane's columns
    _assert_same(nfold.nfold_states(N, s, seeds, tabs, 30, hist=True), want, "N = 32, beta = 0")


def test_the_event_counter_crosses_2_to_the_32_on_the_device():
    N, n = 6, 5
    s = qu.random_boards(N, n, 8)
    seeds = abi.seeds_for(77, n)
    tabs = nfold.weight_tables([0.5, 1.0])
    ev = np.full(n, 2**32 - 3, dtype=np.int64)
    want = nfold.nfold_states_host(N, s, seeds, tabs, 20, events_in=ev, hist=True)
    assert int(want["events_out"].min()) > 2**32 + 2
    _assert_same(nfold.nfold_states(N, s, seeds, tabs, 20, events_in=ev, hist=True), want, "events_in = 2^32 - 3")


def test_in_place_and_the_checks_of_the_wrapper():
    import torch

    dev = torch.device("cuda", torch.cuda.current_device())
    N = 9
    s, seeds, tabs, want = _case(N, "exp")
    t, sd = torch.from_numpy(s).to(dev), torch.from_numpy(seeds.view(np.int32)).to(dev)
    res = nfold.nfold_device(N, t, sd, tabs, STEPS, out=t)
    torch.cuda.current_stream(dev).synchronize()
    assert res["state"] is t and "energy_hist" not in res
    _assert_same(nfold.to_numpy(res), want, "in place", fields=INT_FIELDS)
    with pytest.raises(ValueError, match="seeds"):
        nfold.nfold_device(N, t, sd[:5], tabs, STEPS)
    with pytest.raises(ValueError, match="contiguous uint8 tensor on the GPU"):
        nfold.nfold_device(N, s, sd, tabs, STEPS)
    with pytest.raises(ValueError, match="need_in on the device"):
        nfold.nfold_device(N, t, sd, tabs, STEPS, need_in=torch.zeros(CHAINS, dtype=torch.int32, device=dev))
    with pytest.raises(ValueError, match="out must be"):
        nfold.nfold_device(N, t, sd, tabs, STEPS, out=t[:5])


def test_torch_tensors_on_a_side_stream_in_a_fresh_process(tmp_path):
    """nfold_device on a non-default stream with every input on the device and no synchronise inside: the call returns while a long
    kernel queued before it on the same stream still holds the stream, and the results are right once the stream is waited for."""
    out = str(tmp_path / "n.npz")
    code = f"""
import sys, numpy as np
sys.path.insert(0, {ROOT!r})
import torch, mcq_amd
from tests import quench_util as qu
nfold, abi = mcq_amd.nfold, mcq_amd.abi
dev = torch.device("cuda", 0)
s = qu.random_boards(12, 4099, 77, over=True)
seeds = abi.seeds_for(5, 4099)
tabs = nfold.weight_tables([0.5, 1.0, 2.0])
ln2, ct = nfold.clock_tables("exp")
side = torch.cuda.Stream(dev)
t, sd = torch.from_numpy(s).to(dev), torch.from_numpy(seeds.view(np.int32)).to(dev)
dtab, dct = torch.from_numpy(tabs.view(np.int32)).to(dev), torch.from_numpy(ct.view(np.int32)).to(dev)
nfold.nfold_device(12, t[:8].contiguous(), sd[:8].contiguous(), dtab, 50, clock=(ln2, dct))  # the first launch loads the library's code object
torch.cuda.synchronize()
syncs = []
real = torch.cuda.Stream.synchronize
torch.cuda.Stream.synchronize = lambda self: (syncs.append("stream"), real(self))[1]
real_all = torch.cuda.synchronize
torch.cuda.synchronize = lambda *a, **k: (syncs.append("device"), real_all(*a, **k))[1]
with torch.cuda.stream(side):
    big = torch.empty(1 << 28, dtype=torch.float32, device=dev)
    for _ in range(50):
        big.add_(1.0)  # ~ tens of milliseconds of work ahead of the chains on the side stream
    res = nfold.nfold_device(12, t, sd, dtab, 50, clock=(ln2, dct), hist=True)  # (stream=None: torch's current stream, which is `side`)
    pending = not side.query()
torch.cuda.Stream.synchronize, torch.cuda.synchronize = real, real_all
side.synchronize()
got = nfold.to_numpy(res)
np.savez({out!r}, pending=pending, n_syncs=len(syncs), inp=s, seeds=seeds, tabs=tabs, **got)
"""
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT, timeout=600)
    with np.load(out) as z:
        assert int(z["n_syncs"]) == 0, "nfold_device synchronised"
        assert bool(z["pending"]), "the stream had drained before nfold_device returned: the call cannot be shown to be asynchronous"
        want = nfold.nfold_states_host(12, z["inp"], z["seeds"], z["tabs"], 50, hist=True)
        _assert_same({k: z[k] for k in nfold.FIELDS}, want, "side stream, fresh process")


@pytest.mark.parametrize("init,clock", (("random", "exp"), ("latin", "mean")))
def test_anneal_nfold_is_the_run_composed_from_the_host_code(init, clock):
    N, n, n_steps, seg = 12, 96, 6000, 500
    sp = {"type": "linear_annealing", "beta_start": 1.0, "beta_end": 3.0}
    seeds = abi.seeds_for(42, n)
    got = nfold.anneal_nfold(N, n_steps, init, sp, seeds, seg_steps=seg, clock=clock, hist=True)
    betas = abi.beta_values(sp, n_steps)[::seg]
    assert len(betas) == n_steps // seg and betas[0] == 1.0 and betas[1] == abi.beta_values(sp, n_steps)[seg]
    np.testing.assert_array_equal(got["betas"], betas)
    first, _ = mcq_amd.experiments.start_chains(N, 0, init, sp, seeds, mcmc_type="board", trace=False, states=True)
    start = np.ascontiguousarray(first["final_state"], dtype=np.uint8).reshape(n, -1)
    want = nfold.nfold_states_host(N, start, seeds, nfold.weight_tables(betas), seg, clock=clock, hist=True)
    _assert_same(got, want, f"anneal_nfold, {init}, {clock}")
    np.testing.assert_array_equal(got["energy_in"], first["final_energy"])
    assert (got["best_energy"] < got["energy_in"]).all() and (got["events_out"] < n_steps).all()  # far fewer events than Metropolis steps
    given = nfold.anneal_nfold(N, n_steps, start, sp, seeds, seg_steps=seg, clock=clock, hist=True)
    _assert_same(given, want, "anneal_nfold on given placements")


def test_refused_before_any_launch():
    import torch

    dev = torch.device("cuda", torch.cuda.current_device())
    L = mcq_amd._lib.lib()
    n = 4
    sd = torch.from_numpy(abi.seeds_for(1, n).view(np.int32)).to(dev)
    tabs = nfold.weight_tables([1.0])
    ln2, ct = nfold.clock_tables("exp")
    dtab, dct = torch.from_numpy(tabs.view(np.int32)).to(dev), torch.from_numpy(ct.view(np.int32)).to(dev)
    t33 = torch.zeros((n, 33 * 33), dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError, match=r"N out of range \[2, 32\]: 33"):
        nfold.nfold_device(33, t33, sd, dtab, 10, clock=(ln2, dct))
    with pytest.raises(ValueError, match=r"N out of range \[2, 32\]: 33"):
        nfold.nfold_states(33, np.zeros((n, 33 * 33), dtype=np.uint8), abi.seeds_for(1, n), tabs, 10)
    t = torch.zeros((n, 36), dtype=torch.uint8, device=dev)
    o = torch.full((n, 36), 7, dtype=torch.uint8, device=dev)
    q = nfold._block(6, n, 1, 10, 0, tabs.shape[1], ln2)
    q.mode = abi.MODE_FULL3D
    q.seeds, q.table, q.clock_table, q.state_in, q.state_out = sd.data_ptr(), dtab.data_ptr(), dct.data_ptr(), t.data_ptr(), o.data_ptr()
    assert L.mcq_nfold_device(ctypes.byref(q), None) == abi.EINVAL and b"boards only" in L.mcq_nfold_last_error()
    q.mode, q.N = abi.MODE_BOARD, 33
    assert L.mcq_nfold_device(ctypes.byref(q), None) == abi.EINVAL and b"N out of range" in L.mcq_nfold_last_error()
    torch.cuda.synchronize()
    assert (o.cpu().numpy() == 7).all()  # nothing was launched
