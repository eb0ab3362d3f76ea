"""GPU: the counter form of the tempered board sweep (mcq_temper_counters_device, form="counters") against the library's host code
(mcq_temper_host) and against the lines form (mcq_temper_device) bit for bit on every output, for every N and R it runs; its energies
against the quench kernel's recount after many changed heights; the largest LDS footprint; a caller's own tables; ragged ladder counts;
device segments; torch tensors on a stream of its own; anneal_tempered with either form; and the refusal of N = 17."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import mcq_amd
from tests import heatbath_counters_util as cu
from tests import quench_util as qu
from tests import temper_tables_util as tt
from tests import temper_util as tu

abi = mcq_amd.abi
quench = mcq_amd.quench
tempering = mcq_amd.tempering
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIN = {"type": "linear_annealing", "beta_start": 1.0, "beta_end": 3.0}


def _ladder(R, lo=0.5, hi=2.0):
    return [float(x) for x in np.linspace(lo, hi, R)]


def _boards(N, n, seed):
    """tests/test_heatbath_counters.py's boards: random, one all-equal, one all-255, and where there is room h = (i + j) mod N and
    h = i, which fill whole diagonal lines: the largest counter there can be, N."""
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


def _rungs(n, R, seed):
    rs = np.random.RandomState(seed)
    return np.concatenate([rs.permutation(R) for _ in range(n // R)]).astype(np.uint8)


def _same(got, want, what, hist):
    tu.assert_equal(got, want, what, hist=hist)
    assert set(got) == set(want), what
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)


@pytest.mark.parametrize("N", range(2, 17))
def test_kernel_equals_the_host_code_and_the_lines_kernel(N):
    """Every R; 1, 2 and 3 ladders (two ladders share a workgroup at R = 2: the odd counts leave half of one empty); K = 1, 2, 3; 5 to 7
    sweeps; first_sweep off a multiple of K and beyond 2^34 / N^2; given and default rungs; a beta = 0 row (D = 512, and the most changed
    heights); a steep ladder and an equal one; the histories on (three cases of four) and off."""
    idx = 0
    for R in (2, 4, 8, 16):
        for ladders in (1, 2, 3):
            K, T, trace = 1 + idx % 3, 5 + idx % 3, idx % 4 != 3
            first = (1, 4, (1 << 34) // (N * N) + 5, 7)[idx % 4]
            first += first % K == 0 and K > 1
            betas = np.linspace(0.0, 1.5, T) if idx % 4 == 1 else np.linspace(0.5, 1.6, T)
            ladder = (_ladder(R), _ladder(R), [float(x) for x in np.geomspace(0.05, 6.0, R)], [1.25] * R)[idx % 4]
            n = R * ladders
            s, seeds = _boards(N, n, 10 * N + idx), _seeds(n, N + idx)
            rungs = _rungs(n, R, idx) if idx % 3 else None
            what = f"N={N} R={R}, {ladders} ladders, K={K}, {T} sweeps from {first}, ladder {idx % 4}, rung_in={'given' if idx % 3 else 'default'}"
            assert K == 1 or first % K, what
            want = tempering.temper_states_host(N, s, seeds, betas, ladder, exchange_every=K, first_sweep=first, rungs=rungs, trace=trace)
            got = tempering.temper_states(N, s, seeds, betas, ladder, exchange_every=K, first_sweep=first, rungs=rungs, trace=trace, form="counters")
            _same(got, want, what + ": counters vs the host code", trace)
            lines = tempering.temper_states(N, s, seeds, betas, ladder, exchange_every=K, first_sweep=first, rungs=rungs, trace=trace, form="lines")
            _same(got, lines, what + ": counters vs lines", trace)
            idx += 1
    # against the restatement too, and no sweep at all
    R = (2, 4, 8, 16)[N % 4]
    n = R if N > 8 else 2 * R
    s, seeds = _boards(N, n, 7 * N), _seeds(n, 1)
    got = tempering.temper_states(N, s, seeds, (0.0, 1.2), _ladder(R), exchange_every=1, first_sweep=2, trace=True, form="counters")
    tu.assert_equal(got, tu.run_many(N, s, seeds, (0.0, 1.2), _ladder(R), 1, 2), f"N={N} R={R} vs the restatement", hist=True)
    _same(tempering.temper_states(N, s, seeds, [], _ladder(R), first_sweep=4, trace=True, form="counters"),
          tempering.temper_states_host(N, s, seeds, [], _ladder(R), first_sweep=4, trace=True), f"N={N}, no sweep", True)


@pytest.mark.parametrize("N", (5, 12, 16))
def test_no_drift_after_many_changed_heights(N):
    R, ladders = 16, 2
    n, betas, ladder = R * ladders, [0.0] * 40 + [3.0] * 10, _ladder(R, 0.5, 1.5)
    s, seeds = _boards(N, n, 11 * N), _seeds(n, 5)
    got = tempering.temper_states(N, s, seeds, betas, ladder, exchange_every=2, trace=True, form="counters")
    np.testing.assert_array_equal(quench.quench_states(N, got["state"])["energy_in"], got["energy_out"], err_msg="the quench kernel's recount of state")
    np.testing.assert_array_equal(got["energy_hist"][:, -1], got["energy_out"])
    want = tempering.temper_states_host(N, s, seeds, betas, ladder, exchange_every=2, trace=True)
    assert (want["n_changed"] > 40 * N * N * (N - 1) // N * 0.9).all()  # beta = 0: about (N - 1) / N of 40 N^2 updates changed a height
    _same(got, want, f"N={N}, 50 sweeps", True)
    tu.check_invariants(got, R, 2, 0)


def test_the_largest_lds_footprint():
    """N = 16, R = 16, table_len = 512: 154 816 bytes of LDS per workgroup, the caller's own tables."""
    N, R, K, first, T = 16, 16, 1, 3, 3
    assert abi.temper_counters_lds_bytes(N, R, 512) == 154816
    rs = np.random.RandomState(16)
    tab = -np.sort(-rs.randint(0, (1 << 24) + 1, size=(T, R, 512)), axis=2)  # weights that fall along d, none above 2^24
    tab[:, :, 0] = 1 << 24
    tab = np.ascontiguousarray(tab, dtype=np.uint32)
    X = abi.temper_tables([0.7] * T, _ladder(R), K, first)[1]
    for ladders in (1, 2):
        n = R * ladders
        s, seeds, rungs = _boards(N, n, 16 + ladders), _seeds(n, ladders), _rungs(n, R, ladders)
        want = tu.host_call(N, s, seeds, tab, X, K, first, rungs)
        _same(tt.own_tables(N, s, seeds, tab, X, K, first, rungs), want, f"N=16 R=16 D=512, {ladders} ladders", True)
        assert want["n_changed"].sum() > 0


def test_a_callers_own_tables():
    """A table of one entry (every update uniform), T = [2^24, 0] (only the heights of the smallest count have a weight), and a swap
    table of zeros, with which a pair swaps exactly when Delta >= 0."""
    for N, R in ((2, 16), (9, 4), (16, 2)):
        n, T, K, first = 3 * R, 4, 1, 2
        s, seeds, rungs = _boards(N, n, 7 * N), _seeds(n, 1), _rungs(n, R, N)
        X = abi.temper_tables([0.2] * T, _ladder(R), K, first)[1]
        one = np.full((T, R, 1), 1 << 24, dtype=np.uint32)
        _same(tt.own_tables(N, s, seeds, one, X, K, first, rungs), tu.host_call(N, s, seeds, one, X, K, first, rungs), f"N={N} R={R}, D = 1", True)
        cold = np.tile(np.array([1 << 24, 0], dtype=np.uint32), (T, R, 1))
        got = tt.own_tables(N, s, seeds, cold, X, K, first, rungs)
        _same(got, tu.host_call(N, s, seeds, cold, X, K, first, rungs), f"N={N} R={R}, T = [2^24, 0]", True)
        assert (np.diff(got["energy_hist"], axis=1) <= 0).all()
        Tt = abi.temper_tables(np.linspace(0.3, 1.0, T), _ladder(R), K, first)[0]
        zero = tt.own_tables(N, s, seeds, Tt, np.zeros_like(X), K, first, rungs)
        _same(zero, tu.host_call(N, s, seeds, Tt, np.zeros_like(X), K, first, rungs), f"N={N} R={R}, X = 0", True)
        tu.check_invariants(zero, R, K, first, swap_zero=True)


def test_ragged_ladder_counts_around_one_round_of_workgroups():
    N, R, K = 12, 4, 2
    betas, ladder = (0.0, 0.8, 2.5), _ladder(R)
    for ladders in (1, 255, 257, 1030):
        n = R * ladders
        s, seeds, rungs = _boards(N, n, N + ladders), _seeds(n, ladders), _rungs(n, R, ladders)
        got = tempering.temper_states(N, s, seeds, betas, ladder, exchange_every=K, first_sweep=1, rungs=rungs, trace=True, form="counters")
        lines = tempering.temper_states(N, s, seeds, betas, ladder, exchange_every=K, first_sweep=1, rungs=rungs, trace=True, form="lines")
        _same(got, lines, f"N=12 R=4, {ladders} ladders, counters vs lines", True)
        assert got["n_changed"].sum() > 0 and (ladders == 1 or got["pair_accepted"].sum() > 0)
    # and R = 2, where two ladders share a workgroup, around a round of them
    for ladders in (511, 513):
        n = 2 * ladders
        s, seeds = _boards(N, n, ladders), _seeds(n, 3)
        got = tempering.temper_states(N, s, seeds, betas, [0.5, 1.5], exchange_every=1, trace=True, form="counters")
        lines = tempering.temper_states(N, s, seeds, betas, [0.5, 1.5], exchange_every=1, trace=True, form="lines")
        _same(got, lines, f"N=12 R=2, {ladders} ladders, counters vs lines", True)


def test_device_segments_equal_the_unbroken_launch():
    """In place (state_out == state_in), first_sweep, the rungs and the placements carried on the device, the tables built per segment;
    cuts at sweeps that are and that are not followed by an event."""
    import torch

    dev = torch.device("cuda", torch.cuda.current_device())
    st = torch.cuda.current_stream(dev)
    followed = set()
    for N, R, ladders, K, cuts, first in ((12, 16, 3, 2, (0, 2, 3, 7), 1), (13, 2, 5, 3, (0, 1, 3, 6), 0), (16, 8, 2, 2, (0, 1, 4), (1 << 35) // 256), (5, 4, 1, 1, (0, 2, 3), 5)):
        n, total = R * ladders, cuts[-1]
        betas, ladder = np.linspace(0.3, 1.5, total), _ladder(R)
        s, seeds, rungs = _boards(N, n, 31 * N), _seeds(n, 3), _rungs(n, R, N)
        followed |= {(N, (first + c) % K == 0) for c in cuts[1:-1] if K > 1}
        whole = tempering.temper_states(N, s, seeds, betas, ladder, exchange_every=K, first_sweep=first, rungs=rungs, trace=True, form="counters")
        t, rung = torch.from_numpy(s).to(dev), torch.from_numpy(rungs).to(dev)
        ehist, rhist = [], []
        totals = {k: 0 for k in ("n_changed", "n_exchanges", "pair_accepted")}
        for a, b in zip(cuts[:-1], cuts[1:]):
            res = tempering.temper_device(N, t, seeds, betas[a:b], ladder, exchange_every=K, first_sweep=first + a, rungs=rung, out=t, trace=True, form="counters")
            assert res["state"] is t
            st.synchronize()
            rung = res["rung_out"]
            got = tempering.to_numpy(res)
            ehist.append(got["energy_hist"][:, 0 if a == 0 else 1:]), rhist.append(got["rung_hist"][:, 0 if a == 0 else 1:])
            for k in totals:
                totals[k] = totals[k] + got[k]
        what = f"N={N} R={R} K={K} cuts {cuts}"
        np.testing.assert_array_equal(t.cpu().numpy(), whole["state"], err_msg=what)
        np.testing.assert_array_equal(got["rung_out"], whole["rung_out"], err_msg=what)
        np.testing.assert_array_equal(got["energy_out"], whole["energy_out"], err_msg=what)
        np.testing.assert_array_equal(np.concatenate(ehist, axis=1), whole["energy_hist"], err_msg=what)
        np.testing.assert_array_equal(np.concatenate(rhist, axis=1), whole["rung_hist"], err_msg=what)
        for k in totals:
            np.testing.assert_array_equal(totals[k], whole[k], err_msg=f"{what}: {k}")
    assert {(12, True), (12, False), (13, True), (13, False)} <= followed, followed


def test_torch_tensors_on_a_side_stream_in_a_fresh_process(tmp_path):
    """temper_device(form="counters") on a non-default stream with no synchronise inside: the call returns while a long kernel queued
    before it on the same stream still holds the stream, and the results are right once the stream is waited for."""
    out = str(tmp_path / "t.npz")
    code = f"""
import sys, numpy as np
sys.path.insert(0, {ROOT!r})
import torch, mcq_amd
from tests import quench_util as qu
tempering = mcq_amd.tempering
dev = torch.device("cuda", 0)
N, R, K, first, n = 12, 4, 2, 3, 2052
s = qu.random_boards(N, n, 77, over=True)
seeds = mcq_amd.abi.seeds_for(9, n)
betas, ladder = [0.0, 2.0, 3.0], [0.5, 1.0, 1.5, 2.0]
rungs = np.tile(np.array([2, 0, 3, 1], dtype=np.uint8), n // R)
side = torch.cuda.Stream(dev)
t = torch.from_numpy(s).to(dev)
dseeds = torch.from_numpy(seeds.view(np.int32)).to(dev)
drungs = torch.from_numpy(rungs).to(dev)
tabs = tempering.device_tables(betas, ladder, K, first, dev)
tempering.temper_device(N, t[:8].contiguous(), seeds[:8], betas, ladder, form="counters")  # the first launch loads the library's code object: not part of what is shown
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
    res = tempering.temper_device(N, t, dseeds, tables=tabs, exchange_every=K, first_sweep=first, rungs=drungs, trace=True, form="counters")  # (stream=None: torch's current stream, which is `side`)
    pending = not side.query()
torch.cuda.Stream.synchronize, torch.cuda.synchronize = real, real_all
side.synchronize()
got = tempering.to_numpy(res)
np.savez({out!r}, pending=pending, n_syncs=len(syncs), inp=s, seeds=seeds, rungs=rungs, **got)
"""
    done = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-c", code], cwd=ROOT)
    assert done.returncode == 0, f"the child process ended with status {done.returncode}"
    with np.load(out) as z:
        assert int(z["n_syncs"]) == 0, "temper_device synchronised"
        assert bool(z["pending"]), "the stream had drained before temper_device returned: the call cannot be shown to be asynchronous"
        want = tempering.temper_states_host(12, z["inp"], z["seeds"], [0.0, 2.0, 3.0], [0.5, 1.0, 1.5, 2.0], exchange_every=2, first_sweep=3, rungs=z["rungs"], trace=True)
        tu.assert_equal({k: z[k] for k in tu.FIELDS + ("energy_hist", "rung_hist")}, want, "side stream, fresh process", hist=True)


@pytest.mark.parametrize("mode", (False, True, "pairs"), ids=("plain", "quench", "pairs"))
def test_anneal_tempered_with_counters_equals_lines(mode):
    N, n, n_sweeps = 6, 64, 12
    seeds, start = abi.seeds_for(42, n), qu.random_boards(6, n, 30)
    runs = {form: tempering.anneal_tempered(N, n_sweeps, start, LIN, seeds, _ladder(4, 0.5, 1.5), exchange_every=2, quench=mode, trace=True, form=form)
            for form in tempering.FORMS}
    a, b = runs["counters"], runs["lines"]
    assert set(a) == set(b) and ("quenched_energy" in a) == bool(mode) and ("quench_pair_moves" in a) == (mode == "pairs")
    for k in b:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    assert a["n_changed"].sum() > 0 and a["n_exchanges"].sum() > 0


def test_the_entry_point_refuses_n_17_and_launches_nothing():
    import torch

    N, R, n = 17, 2, 4
    dev = torch.device("cuda", torch.cuda.current_device())
    st = torch.cuda.current_stream(dev)
    T, X = abi.temper_tables([1.0], [1.0, 2.0])
    dT, dX = torch.from_numpy(T.view(np.int32)).to(dev), torch.from_numpy(X.view(np.int32)).to(dev)
    sd = torch.zeros(n, dtype=torch.int32, device=dev)
    t = torch.zeros((n, N * N), dtype=torch.uint8, device=dev)
    o = torch.full((n, N * N), 201, dtype=torch.uint8, device=dev)
    e = torch.full((n,), -77, dtype=torch.int32, device=dev)
    r = torch.full((n,), 99, dtype=torch.uint8, device=dev)
    p = torch.full((n // R, R - 1), -5, dtype=torch.int64, device=dev)
    q = tempering._block(N, n, 1, 0, R, 1, T.shape[2], X.shape[2])
    q.seeds, q.table, q.swap_table, q.state_in, q.state_out = sd.data_ptr(), dT.data_ptr(), dX.data_ptr(), t.data_ptr(), o.data_ptr()
    q.energy_out, q.rung_out, q.pair_accepted = e.data_ptr(), r.data_ptr(), p.data_ptr()
    L = mcq_amd._lib.lib()
    assert L.mcq_temper_counters_device(ctypes.byref(q), ctypes.c_void_p(st.cuda_stream)) == abi.EINVAL
    assert b"16" in L.mcq_temper_last_error(), L.mcq_temper_last_error()
    with pytest.raises(ValueError, match="16"):
        mcq_amd._lib.temper_counters_device(q, st)
    st.synchronize()
    assert (o.cpu().numpy() == 201).all() and (e.cpu().numpy() == -77).all() and (r.cpu().numpy() == 99).all() and (p.cpu().numpy() == -5).all(), "something was launched"
    mcq_amd._lib.temper_device(q, st)  # the lines form takes the same block
    st.synchronize()
    assert (o.cpu().numpy() < N).all() and (e.cpu().numpy() >= 0).all() and (r.cpu().numpy() < R).all() and (p.cpu().numpy() >= 0).all()
