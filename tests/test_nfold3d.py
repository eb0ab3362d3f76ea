"""GPU: the full_3d n-fold kernel (mcq_nfold3d_device) against the library's host code (mcq_nfold3d_host), which follows the definition
pair by pair, bit for bit on every output and dtype at both ends of every instantiation -- 9 chains, 5 segments under rows from
beta = 0 to beta = 8, both clocks, with and without the history, at Q = N^2, a ragged Q and at N <= 4 a cube with one free cell --;
cubes with one free cell in its first and in its last place at N = 4, 12, 13, 19 and 20; seeds whose first event draws a cell of
the first and of the last lane's run at every N; device segments with the need and the event counter
carried on the device against the unbroken launch; a row of zeros that sleeps; the 4096 events of a step under a clock of zeros; the
two cases of wide arithmetic; the largest shape the LDS admits at N = 32; repeated placements among ordinary ones; an event counter that
crosses 2^32; in place; a side stream in a fresh process; anneal_nfold(mcmc_type="full_3d") against the same run composed from the host
code; and what is refused before any launch.  tests/test_nfold3d_host.py holds the host code to the NumPy restatement of the rule."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import mcq_amd
from tests import nfold3d_util as n3
from tests import quench3d_util as q3

abi = mcq_amd.abi
nfold = mcq_amd.nfold
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the instantiations are 64 lanes to N = 12, 256 to N = 19 and 1024 beyond: both ends of each
SIZES = (2, 12, 13, 19, 20, 32)
CHAINS, SEGS = 9, 5
BETAS = (0.0, 0.3, 1.0, 3.0, 8.0)
RAGGED = {2: 3, 12: 37, 13: 11, 19: 23, 20: 7, 32: 5}  # neither a multiple of 64 nor N^2; so few that every lane's run is one queen
INT_FIELDS = tuple(k for k in nfold.FIELDS_3D if k != "energy_hist")


def _shapes(N):
    """(Q, steps per segment): the host code walks Q (N^3 - Q) pairs behind every event, so a few tens of events a chain at N >= 20."""
    big = {2: 40, 12: 40, 13: 40, 19: 12, 20: 10, 32: 8}[N]
    return ((N * N, big), (RAGGED[N], 40 if N < 32 else 25)) + (((N ** 3 - 1, 40),) if N <= 4 else ())


@functools.lru_cache(maxsize=None)
def _tables():
    return nfold.weight_tables(BETAS, abi.MAX_NFOLD3D_TABLE)


@functools.lru_cache(maxsize=None)
def _case(N, Q, steps, clock):
    """(placements with bytes >= N, seeds, the host code's result with the history): computed once, shared and left unchanged."""
    s = q3.random_placements(N, CHAINS, 500 + N + Q, Q=Q, over=True)
    seeds = abi.seeds_for(4000000000 + 100 * N + Q, CHAINS)
    return s, seeds, nfold.nfold_queens_host(N, s, seeds, _tables(), steps, Q=Q, clock=clock, hist=True)


def _assert_same(got, want, what, fields=nfold.FIELDS_3D):
    for k in fields:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].dtype, want[k].dtype)
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{what}: {k}")


@functools.lru_cache(maxsize=None)
def _aimed(N):
    """(placements, seeds, rows, the host code's result) of the two chains of n3.aimed_case at the ragged Q: one step under beta = 0 and
    the mean clock is ONE event each, into a cell of the first lane's run and into one of the last busy lane's run."""
    Q = RAGGED[N]
    s, seeds = n3.aimed_case(N, Q)
    rows = _tables()[:1]
    return s, seeds, rows, nfold.nfold_queens_host(N, s, seeds, rows, 1, Q=Q, clock="mean", hist=True)


def coverage(N):
    """What the comparison at N covers, from the host code's outputs over its shapes and both clocks."""
    cov = dict(up=0, flat=0, better=0, q_first=0, q_last=0, t_first=0, t_last=0, quiet=0)
    for Q, steps in _shapes(N):
        (qa, qb), (qc, qd), (ta, tb), (tc, td) = n3.shares(N, Q)
        for clock in nfold.CLOCKS:
            s, _, want = _case(N, Q, steps, clock)
            cov["quiet"] += int((want["events_out"] == 0).sum())
            cov["up"] += int(want["n_uphill"].sum())
            cov["flat"] += int(want["n_flat"].sum())
            cov["better"] += int(((want["best_energy"] < want["energy_in"]) & (want["best_step"] > 0)).sum())
            q, t = n3.moves(N, s, want["state"])
            cov["q_first"] += int(((q >= qa) & (q < qb)).sum())
            cov["q_last"] += int(((q >= qc) & (q < qd)).sum())
            cov["t_first"] += int(((t >= ta) & (t < tb)).sum())
            cov["t_last"] += int(((t >= tc) & (t < td)).sum())
    s, _, _, want = _aimed(N)
    (_, _, (ta, tb), (tc, td)), (_, t) = n3.shares(N, RAGGED[N]), n3.moves(N, s, want["state"])
    assert (want["events_out"] == 1).all() and len(t) == 2
    cov["t_first"] += int(ta <= t[0] < tb)
    cov["t_last"] += int(tc <= t[1] < td)
    return cov


@pytest.mark.parametrize("N", SIZES)
def test_kernel_equals_the_host_code(N):
    cov = coverage(N)
    print(f"N = {N}: {cov}")
    # events fired in every chain, rises and flat moves occurred, a best below the input exists, and the drawn queen and the drawn cell
    # reached the first and the last lane's share.  (A lane's share of the cube is small beyond N = 12: the two chains of _aimed carry
    # seeds whose first event draws there, and are compared like the others.  N = 2 has one energy per Q: flat moves only.)
    assert cov["quiet"] == 0 and cov["flat"] > 0 and cov["q_first"] > 0 and cov["q_last"] > 0 and (N == 2 or (cov["up"] > 0 and cov["better"] > 0)), cov
    assert cov["t_first"] > 0 and cov["t_last"] > 0, cov
    s, seeds, rows, want = _aimed(N)
    _assert_same(nfold.nfold_queens(N, s, seeds, rows, 1, Q=RAGGED[N], clock="mean", hist=True), want, f"N = {N}: a cell of the first and of the last lane's run")
    for Q, steps in _shapes(N):
        for clock in nfold.CLOCKS:
            s, seeds, want = _case(N, Q, steps, clock)
            got = nfold.nfold_queens(N, s, seeds, _tables(), steps, Q=Q, clock=clock, hist=True)
            _assert_same(got, want, f"N = {N}, Q = {Q}, {clock}")
            slim = nfold.nfold_queens(N, s, seeds, _tables(), steps, Q=Q, clock=clock)
            assert "energy_hist" not in slim
            _assert_same(slim, want, f"N = {N}, Q = {Q}, {clock}, no history", fields=INT_FIELDS)


@pytest.mark.parametrize("N", (4, 12, 13, 19, 20))
def test_a_cube_with_one_free_cell(N):
    """Q = N^3 - 1: every event moves a queen into the one free cell, which is the cube's first cell in chain 0 (the first lane's run)
    and its last in chain 1 (the last busy lane's run, and its last entry); the free cell then wanders."""
    C = N ** 3
    Q = C - 1
    assert abi.nfold3d_lds_bytes(N, Q) <= abi.MAX_NFOLD3D_LDS
    cells = np.arange(C)
    s = np.stack([n3.q3_placement(N, cells[1:]), n3.q3_placement(N, cells[:-1])])
    seeds = abi.seeds_for(77 + N, 2)
    tabs = nfold.weight_tables([0.0, 1.0], abi.MAX_NFOLD3D_TABLE)
    want = nfold.nfold_queens_host(N, s, seeds, tabs, 2, Q=Q, clock="mean", hist=True)
    assert (want["events_out"] >= 2).all() and (want["weight_out"] > 0).all()
    got = nfold.nfold_queens(N, s, seeds, tabs, 2, Q=Q, clock="mean", hist=True)
    _assert_same(got, want, f"one free cell, N = {N}")
    one = nfold.nfold_queens_host(N, s, seeds, tabs[:1], 1, Q=Q, clock="mean")  # one event each: into cell 0, into cell C - 1
    q, t = n3.moves(N, s, one["state"])
    assert (one["events_out"] == 1).all() and sorted(int(v) for v in t) == [0, C - 1]
    _assert_same(nfold.nfold_queens(N, s, seeds, tabs[:1], 1, Q=Q, clock="mean"), one, f"one event, N = {N}", fields=INT_FIELDS)


@pytest.mark.parametrize("N", (5, 13, 20))
def test_segments_carried_on_the_device_are_the_unbroken_launch(N):
    import torch

    dev = torch.device("cuda", torch.cuda.current_device())
    Q, steps = N * N, 10
    s, seeds, want = _case(N, Q, steps, "exp")
    tabs = _tables()
    t, sd = torch.from_numpy(s).to(dev), torch.from_numpy(seeds.view(np.int32)).to(dev)
    dtab = torch.from_numpy(tabs.view(np.int32)).to(dev)
    ln2, ct = nfold.clock_tables("exp")
    clock = (ln2, torch.from_numpy(ct.view(np.int32)).to(dev))
    state, need, events, pieces = t, None, None, []
    for first, last in ((0, 1), (1, 1), (1, 3), (3, 5)):  # a piece of no segment among them; nothing is copied back in between
        res = nfold.nfold_queens_device(N, state, sd, dtab[first:last], steps, first_seg=first, clock=clock, need_in=need, events_in=events, hist=True)
        state, need, events = res["state"], res["need_out"], res["events_out"]
        pieces.append(res)
    torch.cuda.current_stream(dev).synchronize()
    out = [nfold.to_numpy(p) for p in pieces]
    for k in ("state", "energy_out", "events_out", "need_out", "weight_out", "flags"):
        np.testing.assert_array_equal(out[-1][k], want[k], err_msg=k)
    np.testing.assert_array_equal(np.concatenate([out[0]["energy_hist"]] + [o["energy_hist"][:, 1:] for o in out[1:]], axis=1), want["energy_hist"])
    np.testing.assert_array_equal(sum(o["n_uphill"] for o in out), want["n_uphill"])
    np.testing.assert_array_equal(sum(o["n_flat"] for o in out), want["n_flat"])
    best = np.minimum.reduce([o["best_energy"] for o in out])
    np.testing.assert_array_equal(best, want["best_energy"])
    starts = (0, 1, 1, 3)
    step = np.full(CHAINS, -1, dtype=np.int64)
    for o, first in reversed(list(zip(out, starts))):  # the first piece that holds the best
        step = np.where(o["best_energy"] == best, o["best_step"] + first * steps, step)
    np.testing.assert_array_equal(step, want["best_step"])
    np.testing.assert_array_equal(t.cpu().numpy(), s)  # out of place: the input is untouched


def test_a_row_of_zeros_sleeps_on_the_device():
    N, Q, n = 6, 20, 7
    s = q3.random_placements(N, n, 6, Q=Q)
    rows = np.zeros((3, 4), dtype=np.uint32)
    need = (np.arange(n, dtype=np.uint64) * 12345 + 1) << 33
    ev = np.arange(n, dtype=np.int64) + 2**33
    want = nfold.nfold_queens_host(N, s, abi.seeds_for(5, n), rows, 1 << 31, Q=Q, need_in=need, events_in=ev, hist=True)
    got = nfold.nfold_queens(N, s, abi.seeds_for(5, n), rows, 1 << 31, Q=Q, need_in=need, events_in=ev, hist=True)
    _assert_same(got, want, "a row of zeros")
    np.testing.assert_array_equal(got["need_out"], need)
    np.testing.assert_array_equal(got["events_out"], ev)
    np.testing.assert_array_equal(got["state"], s)
    assert (got["weight_out"] == 0).all() and (got["energy_hist"] == got["energy_in"][:, None]).all()


def test_a_clock_of_zeros_fires_4096_events_per_step_on_the_device():
    N, Q, n, S = 3, 3, 9, 2
    s = q3.random_placements(N, n, 12, Q=Q)
    seeds = abi.seeds_for(31, n)
    tabs = nfold.weight_tables([0.0] * S, abi.MAX_NFOLD3D_TABLE)
    zero = (0, np.zeros(256, dtype=np.uint32))
    got = nfold.nfold_queens(N, s, seeds, tabs, 1, Q=Q, clock=zero, hist=True)
    assert (got["events_out"] == S << abi.NFOLD_TIME_BITS).all() and (got["need_out"] == 0).all()
    assert (got["weight_out"] == Q * (N ** 3 - Q) << 24).all()
    _assert_same(got, nfold.nfold_queens_host(N, s, seeds, tabs, 1, Q=Q, clock=zero, hist=True), "a clock of zeros")


def test_wide_arithmetic_a_need_beyond_2_to_the_52():
    """N = 32, Q = 1 024 under the row [1, 0]: W is the number of moves that do not raise E, about 2^24, so a need near 2^58 has
    need 2^12 >= 2^64 and q1 >= 2^32, and a segment of 2^31 steps takes the 96-bit product of the branch that does not fire; a need of
    about 2^31 W fires just before the segment ends, with q1 < 2^32 and the second quotient."""
    s, seeds, need, rows, want = n3.wide_need_case(nfold, abi)
    assert (want["events_out"][:3] == 0).all() and want["events_out"][3] >= 1 and (want["need_out"][:3] < need[:3]).all()
    got = nfold.nfold_queens(32, s, seeds, rows, 1 << 31, clock="mean", need_in=need, hist=True)
    _assert_same(got, want, "a need beyond 2^52")


@functools.lru_cache(maxsize=None)
def _largest():
    """The largest shape the LDS admits at N = 32 under beta = 0: W = M 2^24 at the largest M, where U takes the whole 128-bit product."""
    N = 32
    Q = n3.largest_queens(abi, N)
    s = q3.random_placements(N, 2, 5, Q=Q)
    seeds = abi.seeds_for(4294967000, 2)
    tabs = nfold.weight_tables([0.0], abi.MAX_NFOLD3D_TABLE)
    return N, Q, s, seeds, tabs, nfold.nfold_queens_host(N, s, seeds, tabs, 3, Q=Q, clock="mean", hist=True)


def test_the_largest_shape_of_the_lds_with_every_weight_at_its_bound():
    N, Q, s, seeds, tabs, want = _largest()
    assert abi.nfold3d_lds_bytes(N, Q) <= abi.MAX_NFOLD3D_LDS < abi.nfold3d_lds_bytes(N, Q + 1)
    assert (want["weight_out"] == Q * (N ** 3 - Q) << 24).all() and (want["events_out"] == 3).all()
    _assert_same(nfold.nfold_queens(N, s, seeds, tabs, 3, Q=Q, clock="mean", hist=True), want, f"N = 32, Q = {Q}, beta = 0")


def test_repeated_placements_among_ordinary_ones():
    N, Q, n = 6, 36, 8
    s = q3.random_placements(N, n, 9, Q=Q, over=True)
    s[2, 3:6] = s[2, 0:3]  # queens 0 and 1 in one cell
    s[5, 3 * (Q - 1):] = s[5, 30:33]
    s[6] = 200  # every queen clamped into the last cell
    seeds = abi.seeds_for(3, n)
    tabs = _tables()
    need = np.arange(1, n + 1, dtype=np.uint64) << 40
    ev = np.arange(n, dtype=np.int64) * 7
    for kw in (dict(), dict(need_in=need, events_in=ev)):
        want = nfold.nfold_queens_host(N, s, seeds, tabs, 20, clock="exp", hist=True, **kw)
        assert [int(f) for f in want["flags"]] == [0, 0, 1, 0, 0, 1, 1, 0] and want["energy_out"][6] == Q * (Q - 1) // 2
        got = nfold.nfold_queens(N, s, seeds, tabs, 20, clock="exp", hist=True, **kw)
        _assert_same(got, want, f"repeated placements {sorted(kw)}")
        rep = want["flags"] == 1
        np.testing.assert_array_equal(got["state"][rep], np.minimum(s, N - 1)[rep])
        np.testing.assert_array_equal(got["best_state"][rep], np.minimum(s, N - 1)[rep])
        assert (got["weight_out"][rep] == 0).all() and (got["events_out"][rep] == (ev[rep] if kw else 0)).all()
        if kw:
            np.testing.assert_array_equal(got["need_out"][rep], need[rep])


def test_the_event_counter_crosses_2_to_the_32_on_the_device():
    N, Q, n = 6, 30, 5
    s = q3.random_placements(N, n, 8, Q=Q)
    seeds = abi.seeds_for(77, n)
    tabs = nfold.weight_tables([0.5, 1.0], abi.MAX_NFOLD3D_TABLE)
    ev = np.full(n, 2**32 - 3, dtype=np.int64)
    want = nfold.nfold_queens_host(N, s, seeds, tabs, 20, Q=Q, events_in=ev, hist=True)
    assert int(want["events_out"].min()) > 2**32 + 2
    _assert_same(nfold.nfold_queens(N, s, seeds, tabs, 20, Q=Q, events_in=ev, hist=True), want, "events_in = 2^32 - 3")


def test_in_place_and_the_checks_of_the_wrapper():
    import torch

    dev = torch.device("cuda", torch.cuda.current_device())
    N, Q, steps = 13, 169, 40
    s, seeds, want = _case(N, Q, steps, "exp")
    t, sd = torch.from_numpy(s).to(dev), torch.from_numpy(seeds.view(np.int32)).to(dev)
    res = nfold.nfold_queens_device(N, t, sd, _tables(), steps, out=t)
    torch.cuda.current_stream(dev).synchronize()
    assert res["state"] is t and "energy_hist" not in res
    _assert_same(nfold.to_numpy(res), want, "in place", fields=INT_FIELDS)
    # a stream handed over by name: every upload and the kernel go there, behind what the current stream has done so far
    t2, side = torch.from_numpy(s).to(dev), torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    on_side = nfold.nfold_queens_device(N, t2, sd, _tables(), steps, hist=True, stream=side)
    side.synchronize()
    _assert_same(nfold.to_numpy(on_side), want, "stream=side")
    with pytest.raises(ValueError, match="seeds"):
        nfold.nfold_queens_device(N, t, sd[:5], _tables(), steps)
    with pytest.raises(ValueError, match="contiguous uint8 tensor on the GPU"):
        nfold.nfold_queens_device(N, s, sd, _tables(), steps)
    with pytest.raises(ValueError, match="need_in on the device"):
        nfold.nfold_queens_device(N, t, sd, _tables(), steps, need_in=torch.zeros(CHAINS, dtype=torch.int32, device=dev))
    with pytest.raises(ValueError, match="out must be"):
        nfold.nfold_queens_device(N, t, sd, _tables(), steps, out=t[:5])
    with pytest.raises(ValueError, match="final_state layout of full_3d"):
        nfold.nfold_queens_device(N, t, sd, _tables(), steps, Q=Q + 1)


def test_torch_tensors_on_a_side_stream_in_a_fresh_process(tmp_path):
    """nfold_queens_device on a non-default stream with every input on the device and no synchronise inside: the call returns while a
    long kernel queued before it on the same stream still holds the stream, and the results are right once the stream is waited for."""
    out = str(tmp_path / "n.npz")
    code = f"""
import sys, numpy as np
sys.path.insert(0, {ROOT!r})
import torch, mcq_amd
from tests import quench3d_util as q3
nfold, abi = mcq_amd.nfold, mcq_amd.abi
dev = torch.device("cuda", 0)
n = 131
s = q3.random_placements(8, n, 77, over=True)
seeds = abi.seeds_for(5, n)
tabs = nfold.weight_tables([0.5, 1.0, 2.0], abi.MAX_NFOLD3D_TABLE)
ln2, ct = nfold.clock_tables("exp")
side = torch.cuda.Stream(dev)
t, sd = torch.from_numpy(s).to(dev), torch.from_numpy(seeds.view(np.int32)).to(dev)
dtab, dct = torch.from_numpy(tabs.view(np.int32)).to(dev), torch.from_numpy(ct.view(np.int32)).to(dev)
nfold.nfold_queens_device(8, t[:8].contiguous(), sd[:8].contiguous(), dtab, 30, clock=(ln2, dct))  # the first launch loads the library's code object
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
    res = nfold.nfold_queens_device(8, t, sd, dtab, 30, clock=(ln2, dct), hist=True)  # (stream=None: torch's current stream, which is `side`)
    pending = not side.query()
torch.cuda.Stream.synchronize, torch.cuda.synchronize = real, real_all
side.synchronize()
got = nfold.to_numpy(res)
np.savez({out!r}, pending=pending, n_syncs=len(syncs), inp=s, seeds=seeds, tabs=tabs, **got)
"""
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT, timeout=600)
    with np.load(out) as z:
        assert int(z["n_syncs"]) == 0, "nfold_queens_device synchronised"
        assert bool(z["pending"]), "the stream had drained before nfold_queens_device returned: the call cannot be shown to be asynchronous"
        want = nfold.nfold_queens_host(8, z["inp"], z["seeds"], z["tabs"], 30, hist=True)
        _assert_same({k: z[k] for k in nfold.FIELDS_3D}, want, "side stream, fresh process")


@pytest.mark.parametrize("init,clock", (("random", "exp"), ("latin", "mean")))
def test_anneal_nfold_full_3d_is_the_run_composed_from_the_host_code(init, clock):
    N, n, n_steps, seg = 6, 24, 3000, 250
    sp = {"type": "linear_annealing", "beta_start": 1.0, "beta_end": 3.0}
    seeds = abi.seeds_for(42, n)
    got = nfold.anneal_nfold(N, n_steps, init, sp, seeds, seg_steps=seg, clock=clock, hist=True, mcmc_type="full_3d")
    betas = abi.beta_values(sp, n_steps)[::seg]
    assert len(betas) == n_steps // seg and betas[0] == 1.0 and betas[1] == abi.beta_values(sp, n_steps)[seg]
    np.testing.assert_array_equal(got["betas"], betas)
    first, _ = mcq_amd.experiments.start_chains(N, 0, init, sp, seeds, mcmc_type="full_3d", trace=False, states=True)
    start = np.ascontiguousarray(first["final_state"], dtype=np.uint8).reshape(n, -1)
    assert start.shape == (n, 3 * N * N)
    want = nfold.nfold_queens_host(N, start, seeds, nfold.weight_tables(betas, abi.MAX_NFOLD3D_TABLE), seg, clock=clock, hist=True)
    _assert_same(got, want, f"anneal_nfold full_3d, {init}, {clock}")
    np.testing.assert_array_equal(got["energy_in"], first["final_energy"])
    assert (got["events_out"] > 0).all() and (got["events_out"] < n_steps).all()  # fewer events than Metropolis steps
    given = nfold.anneal_nfold(N, n_steps, start, sp, seeds, seg_steps=seg, clock=clock, hist=True, mcmc_type="full_3d")
    _assert_same(given, want, "anneal_nfold full_3d on given placements")


def test_refused_before_any_launch():
    import torch

    dev = torch.device("cuda", torch.cuda.current_device())
    L = mcq_amd._lib.lib()
    n = 4
    sd = torch.from_numpy(abi.seeds_for(1, n).view(np.int32)).to(dev)
    tabs = nfold.weight_tables([1.0], abi.MAX_NFOLD3D_TABLE)
    ln2, ct = nfold.clock_tables("exp")
    dtab, dct = torch.from_numpy(tabs.view(np.int32)).to(dev), torch.from_numpy(ct.view(np.int32)).to(dev)
    t33 = torch.zeros((n, 3 * 33 * 33), dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError, match=r"N out of range \[2, 32\]: 33"):
        nfold.nfold_queens_device(33, t33, sd, dtab, 10, clock=(ln2, dct))
    Qbig = n3.largest_queens(abi, 32) + 1
    size = 3 * Qbig
    t = torch.zeros((n, size), dtype=torch.uint8, device=dev)
    o = torch.full((n, size), 7, dtype=torch.uint8, device=dev)

    def block(N, Q, mode=abi.MODE_FULL3D):
        q = nfold._block3d(N, Q, n, 1, 10, 0, tabs.shape[1], ln2)
        q.mode = mode
        q.seeds, q.table, q.clock_table, q.state_in, q.state_out = sd.data_ptr(), dtab.data_ptr(), dct.data_ptr(), t.data_ptr(), o.data_ptr()
        return q

    for q, msg in ((block(33, 0), b"N out of range [2, 32]: 33"), (block(6, 1), b"n_queens out of range [2, N^3 - 1 = 215] (0 = N^2): 1"),
                   (block(6, 216), b"n_queens out of range [2, N^3 - 1 = 215] (0 = N^2): 216"), (block(6, 0, abi.MODE_BOARD), b"full_3d placements only"),
                   (block(32, Qbig), f"N = 32 with n_queens = {Qbig}: a chain takes {abi.nfold3d_lds_bytes(32, Qbig)} bytes of LDS".encode())):
        assert L.mcq_nfold3d_device(ctypes.byref(q), None) == abi.EINVAL and msg in L.mcq_nfold3d_last_error(), (msg, L.mcq_nfold3d_last_error())
    with pytest.raises(ValueError, match=f"N = 32 with n_queens = {Qbig}"):
        nfold.nfold_queens_device(32, t, sd, dtab, 10, Q=Qbig, clock=(ln2, dct), out=o)
    torch.cuda.synchronize()
    assert (o.cpu().numpy() == 7).all()  # nothing was launched
    # the NumPy wrapper hands such a shape to the host code instead
    s = q3.random_placements(32, 1, 3, Q=Qbig)
    row = np.zeros((1, 2), dtype=np.uint32)  # (a row of zeros: the recount, no pair is walked twice)
    np.testing.assert_array_equal(nfold.nfold_queens(32, s, abi.seeds_for(1, 1), row, 1, Q=Qbig)["state"], s)
