"""GPU: the heat-bath kernel (mcq_heatbath_device) against the library's host code (mcq_heatbath_host) bit for bit on every output, its
energies against the quench kernel's recount, device segments against the unbroken call, anneal_heatbath with resampling against a run
composed on the host, behind the competition driver, and on torch tensors on a stream of its own."""
import os
import subprocess
import sys

import numpy as np
import pytest

import mcq_amd
from tests import heatbath_util as hu
from tests import population_util as pu
from tests import quench_util as qu
from tests import resume_util as ru

abi = mcq_amd.abi
heatbath = mcq_amd.heatbath
quench = mcq_amd.quench
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIN = {"type": "linear_annealing", "beta_start": 1.0, "beta_end": 3.0}

# every instantiation (line paddings 8, 12, 16, 24, 32, 64, 128; 16, 32, 64 lanes; two heights per lane beyond N = 64)
SIZES = (2, 3, 8, 12, 13, 16, 17, 24, 32, 33, 64, 65, 128)
BETAS = ((0.0, 3.0, 1.0), (0.5, 0.5), (3.0,), (1.0, 2.0, 2.5, 3.0), (0.004,))


def _boards(N, n, seed):
    s = qu.random_boards(N, n, seed, over=seed % 2 == 1)
    s[0] = seed % N  # all heights equal
    if n > 2:
        s[1] = 255  # clamped
    return s


def _seeds(n, k):
    s = (np.arange(n, dtype=np.uint64) * 2654435761 + k) % 2**32
    s[-1] = 2**32 - 1
    return s.astype(np.uint32)


@pytest.mark.parametrize("N", SIZES)
def test_kernel_equals_the_host_code(N):
    counts = (1, 3, 5, 17) if N <= 33 else (1, 3, 5) if N <= 65 else (1, 3)
    for idx, n in enumerate(counts):
        for t, betas in enumerate(BETAS if idx < 2 and N <= 33 else BETAS[idx % 3: idx % 3 + 1]):
            if N > 33:
                betas = betas[:2]
            first = (0, 3, (1 << 34) // (N * N) + 5, 1 << 40)[(idx + t) % 4]
            trace = (idx + t) % 2 == 0
            s, seeds = _boards(N, n, 100 * N + idx), _seeds(n, N + t)
            want = heatbath.heatbath_states_host(N, s, seeds, betas, first_sweep=first, trace=trace)
            got = heatbath.heatbath_states(N, s, seeds, betas, first_sweep=first, trace=trace)
            hu.assert_equal(got, want, f"N={N}, {n} chains, betas={betas}, first_sweep={first}", hist=trace)
            assert set(got) == set(want)
            for k in want:
                assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
    # a table of one entry (uniform updates) and no sweep at all
    s, seeds = _boards(N, 3, 7 * N), _seeds(3, 1)
    hu.assert_equal(heatbath.heatbath_states(N, s, seeds, [], first_sweep=4), heatbath.heatbath_states_host(N, s, seeds, [], first_sweep=4), f"N={N}, no sweep")
    hu.assert_equal(heatbath.heatbath_states(N, s, seeds, [50.0]), heatbath.heatbath_states_host(N, s, seeds, [50.0]), f"N={N}, beta = 50")
    # against the restatement too, where it is quick
    if N <= 17:
        hu.assert_equal(heatbath.heatbath_states(N, s, seeds, (1.0, 3.0), first_sweep=2, trace=True), hu.sweeps_many(N, s, seeds, (1.0, 3.0), 2),
                        f"N={N} vs the restatement", hist=True)


def test_ragged_chain_counts_around_the_wavefront():
    for N, counts in ((12, (2, 4, 6, 7, 63, 64, 65, 1025)), (8, (255, 257)), (24, (2, 31, 33)), (40, (2, 9)), (70, (2,))):
        for n in counts:
            s, seeds = _boards(N, n, N + n), _seeds(n, n)
            betas = (1.0, 2.5)
            want = heatbath.heatbath_states_host(N, s, seeds, betas, first_sweep=n, trace=True)
            got = heatbath.heatbath_states(N, s, seeds, betas, first_sweep=n, trace=True)
            hu.assert_equal(got, want, f"N={N}, {n} chains", hist=True)


def test_many_chains_and_the_quench_kernels_recount():
    import torch

    N, n, betas = 12, 65536, np.linspace(1.0, 3.0, 4)
    s, seeds = qu.random_boards(N, n, 12), abi.seeds_for(42, n)
    dev = torch.device("cuda", torch.cuda.current_device())
    res = heatbath.heatbath_device(N, torch.from_numpy(s).to(dev), seeds, betas, trace=True)
    again = quench.quench_device(N, res["state"], max_passes=1, conflicts=False)
    best = quench.quench_device(N, res["best_state"], max_passes=1, conflicts=False)
    torch.cuda.current_stream(dev).synchronize()
    got = heatbath.to_numpy(res)
    np.testing.assert_array_equal(again["energy_in"].cpu().numpy(), got["energy_out"], err_msg="the quench kernel's recount of state_out")
    np.testing.assert_array_equal(best["energy_in"].cpu().numpy(), got["best_energy"], err_msg="the quench kernel's recount of best_state")
    np.testing.assert_array_equal(got["energy_hist"].min(axis=1), got["best_energy"])
    np.testing.assert_array_equal(got["energy_hist"].argmin(axis=1), got["best_sweep"])
    pick = np.r_[0:40, n // 2: n // 2 + 40, n - 40: n]
    want = heatbath.heatbath_states_host(N, s[pick], seeds[pick], betas, trace=True)
    hu.assert_equal({k: v[pick] for k, v in got.items()}, want, "a sample of 65 536 chains", hist=True)
    share = got["n_changed"].sum() / (n * len(betas) * N * N)
    print(f"N=12, 65 536 chains, 4 sweeps 1 -> 3: energy {got['energy_in'].mean():.1f} -> {got['energy_out'].mean():.1f}, changed updates {share:.3f}")
    assert (got["energy_out"] < got["energy_in"]).mean() > 0.99 and 0.0 < share < 1.0


def test_device_segments_equal_the_unbroken_call():
    import torch

    dev = torch.device("cuda", torch.cuda.current_device())
    st = torch.cuda.current_stream(dev)
    for N, n, cuts, first in ((12, 37, (0, 2, 3, 7), 0), (20, 9, (0, 1, 4), (1 << 35) // 400), (70, 3, (0, 1, 2), 5)):
        total = cuts[-1]
        betas = np.linspace(0.5, 3.0, total)
        s, seeds = _boards(N, n, 31 * N), _seeds(n, 3)
        whole = heatbath.heatbath_states(N, s, seeds, betas, first_sweep=first, trace=True)
        t = torch.from_numpy(s).to(dev)
        hist = [None] * (total + 1)
        for a, b in zip(cuts[:-1], cuts[1:]):
            res = heatbath.heatbath_device(N, t, seeds, betas[a:b], first_sweep=first + a, out=t, trace=True)  # in place
            assert res["state"] is t
            st.synchronize()
            h = res["energy_hist"].cpu().numpy()
            if a > 0:
                np.testing.assert_array_equal(h[:, 0], hist[a], err_msg=f"N={N}: the recount at sweep {a}")
            for e in range(b - a + 1):
                hist[a + e] = h[:, e]
        np.testing.assert_array_equal(t.cpu().numpy(), whole["state"], err_msg=f"N={N}: segments {cuts}")
        np.testing.assert_array_equal(np.stack(hist, axis=1), whole["energy_hist"], err_msg=f"N={N}: joined history")
        # only the placements: every per-chain output is optional, and out of place leaves the input alone
        q = abi.Heatbath()
        t2, o2 = torch.from_numpy(s).to(dev), torch.zeros((n, N * N), dtype=torch.uint8, device=dev)
        tab = torch.from_numpy(abi.heatbath_table(betas).view(np.int32)).to(dev)
        sd = torch.from_numpy(seeds.view(np.int32)).to(dev)
        q.N, q.mode, q.n_chains, q.n_sweeps, q.first_sweep, q.table_len = N, abi.MODE_BOARD, n, total, first, tab.shape[1]
        q.seeds, q.table, q.state_in, q.state_out = sd.data_ptr(), tab.data_ptr(), t2.data_ptr(), o2.data_ptr()
        mcq_amd._lib.heatbath_device(q, st)
        st.synchronize()
        np.testing.assert_array_equal(o2.cpu().numpy(), whole["state"])
        np.testing.assert_array_equal(t2.cpu().numpy(), s)


def _compose_host(N, n_sweeps, start, sp, seeds, S, population, resample_seed, trace):
    """The run anneal_heatbath makes, composed on the host: heatbath_states_host segments, population_util.plan in between."""
    n = len(seeds)
    R = n if population is None else population
    K = -(-n_sweeps // S)
    lengths = [S] * (K - 1) + [n_sweeps - (K - 1) * S]
    beta = abi.beta_values(sp, n_sweeps)
    offsets = np.random.RandomState(resample_seed).randint(0, 2**32, size=(K - 1, n // R), dtype=np.uint32)
    state, done = start, 0
    segs, parents, stats, received = [], [], [], []
    best = None
    hist = np.zeros((n, n_sweeps + 1), dtype=np.int32)
    for k, L in enumerate(lengths):
        seg = heatbath.heatbath_states_host(N, state, seeds, beta[done: done + L], first_sweep=done, trace=True)
        segs.append(seg)
        if k == 0:
            best = {"best_energy": seg["best_energy"].copy(), "best_sweep": seg["best_sweep"].copy(), "best_state": seg["best_state"].copy(),
                    "n_changed": seg["n_changed"].copy()}
            hist[:, : L + 1] = seg["energy_hist"]
        else:
            lower = seg["best_energy"] < best["best_energy"]
            best["best_energy"][lower] = seg["best_energy"][lower]
            best["best_sweep"][lower] = seg["best_sweep"][lower] + done
            best["best_state"][lower] = seg["best_state"][lower]
            best["n_changed"] += seg["n_changed"]
            hist[:, done + 1: done + L + 1] = seg["energy_hist"][:, 1:]
        if k < K - 1:
            par, stt = pu.plan(seg["energy_out"], R, pu.table(beta[(k + 1) * S] - beta[k * S]), offsets[k])
            state = seg["state"][par]
            parents.append(par), stats.append(stt), received.append(seg["energy_out"][par])
        done += L
    res = dict(best, initial_energy=segs[0]["energy_in"], final_energy=segs[-1]["energy_out"], final_state=segs[-1]["state"])
    if trace:
        res["energy_hist"] = hist
    par = np.array(parents, dtype=np.int32).reshape(K - 1, n)
    sts = np.array(stats, dtype=np.int64).reshape(K - 1, n // R, 3)
    anc = np.arange(n, dtype=np.int32)
    for q in par:
        anc = anc[q]
    lineage = {"parents": par, "distinct_parents": sts[:, :, 0], "weight_sum": sts[:, :, 1], "e_min": sts[:, :, 2], "ancestors": anc,
               "segment_initial_energy": np.array([s["energy_in"] for s in segs]), "segment_final_energy": np.array([s["energy_out"] for s in segs]),
               "received_energy": np.array(received, dtype=np.int32).reshape(K - 1, n)}
    return res, lineage


RES_FIELDS = ("initial_energy", "final_energy", "final_state", "best_energy", "best_sweep", "best_state", "n_changed")


@pytest.mark.parametrize("N,n,R,n_sweeps,S,trace", ((6, 64, 32, 23, 5, True), (6, 64, None, 20, 5, False), (12, 96, 48, 17, 4, True), (12, 96, 16, 12, 12, False)))
def test_anneal_heatbath_equals_the_run_composed_on_the_host(N, n, R, n_sweeps, S, trace):
    seeds = abi.seeds_for(42, n)
    start = qu.random_boards(N, n, 5 * N)
    got, lin = heatbath.anneal_heatbath(N, n_sweeps, start, LIN, seeds, resample_every=S, population=R, resample_seed=3, trace=trace)
    want, wlin = _compose_host(N, n_sweeps, start, LIN, seeds, S, R, 3, trace)
    what = f"N={N} {n} chains in populations of {R}, {n_sweeps} sweeps cut every {S}"
    for k in RES_FIELDS + (("energy_hist",) if trace else ()):
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{what}: {k}")
    assert ("energy_hist" in got) == trace
    for k in pu.LINEAGE_FIELDS:
        np.testing.assert_array_equal(lin[k], wlin[k], err_msg=f"{what}: lineage {k}")
    assert lin["lengths"] == [S] * (len(lin["lengths"]) - 1) + [n_sweeps - S * (len(lin["lengths"]) - 1)] and lin["population"] == (R or n)
    if n_sweeps > S:
        assert (lin["distinct_parents"] < lin["population"]).any(), "no boundary resampled anything"


def test_constant_schedule_and_init_modes():
    """dbeta = 0 makes every resampling the identity: the run equals the one without resampling.  An init mode gives the reference's
    own initial placements (those of the Metropolis chains with the same seeds)."""
    const = {"type": "constant", "beta_const": 1.5}
    seeds = abi.seeds_for(7, 64)
    start = qu.random_boards(12, 64, 2)
    plain = heatbath.anneal_heatbath(12, 9, start, const, seeds, trace=True)
    res, lin = heatbath.anneal_heatbath(12, 9, start, const, seeds, resample_every=2, population=32, trace=True)
    assert set(plain) == set(res)
    for k, v in plain.items():
        np.testing.assert_array_equal(res[k], v, err_msg=f"{k}: identity resampling changed the run")
    np.testing.assert_array_equal(lin["parents"], np.tile(np.arange(64, dtype=np.int32), (4, 1)))
    hu.assert_equal({"state": plain["final_state"], "energy_in": plain["initial_energy"], "energy_out": plain["final_energy"], "best_energy": plain["best_energy"],
                     "best_sweep": plain["best_sweep"], "best_state": plain["best_state"], "n_changed": plain["n_changed"], "energy_hist": plain["energy_hist"]},
                    heatbath.heatbath_states_host(12, start, seeds, [1.5] * 9, trace=True), "anneal_heatbath without resampling", hist=True)
    for mode in ("random", "latin", "klarner"):
        res = heatbath.anneal_heatbath(7, 0, mode, LIN, seeds)
        first, _ = mcq_amd._lib.run_host(abi.make_params(7, 1, mode, LIN, 64, mcmc_type="board"), seeds, trace=False)
        np.testing.assert_array_equal(res["initial_energy"], first["initial_energy"], err_msg=mode)
        np.testing.assert_array_equal(res["final_state"], res["best_state"])
        assert ru.recount("board", 7, res["final_state"][5]) == int(res["final_energy"][5]) == int(first["initial_energy"][5])
        went = heatbath.anneal_heatbath(7, 6, mode, LIN, seeds)
        hu.assert_equal({"state": went["final_state"], "energy_in": went["initial_energy"], "energy_out": went["final_energy"], "best_energy": went["best_energy"],
                         "best_sweep": went["best_sweep"], "best_state": went["best_state"], "n_changed": went["n_changed"]},
                        heatbath.heatbath_states_host(7, res["final_state"], seeds, abi.beta_values(LIN, 6)), f"init {mode}")


def test_quench_and_the_competition_driver(tmp_path):
    seeds = abi.seeds_for(42, 128)
    kw = dict(resample_every=5, population=64, resample_seed=1)
    plain, lin0 = heatbath.anneal_heatbath(12, 30, "random", LIN, seeds, **kw)
    res, lin1 = heatbath.anneal_heatbath(12, 30, "random", LIN, seeds, quench=True, **kw)
    new = {"quenched_state", "quenched_energy", "quench_moves"}
    assert set(res) == set(plain) | new and not (new & set(plain))
    for k, v in plain.items():
        np.testing.assert_array_equal(res[k], v, err_msg=f"{k} changed with quench=True")
    for k in pu.LINEAGE_FIELDS:
        np.testing.assert_array_equal(lin1[k], lin0[k], err_msg=f"lineage {k}")
    want = quench.quench_states(12, res["best_state"])
    np.testing.assert_array_equal(res["quenched_state"], want["state"])
    np.testing.assert_array_equal(res["quenched_energy"], want["energy_out"])
    np.testing.assert_array_equal(res["quench_moves"], want["n_moves"])
    np.testing.assert_array_equal(want["energy_in"], res["best_energy"])
    second = quench.quench_states(12, res["quenched_state"])
    assert not second["n_moves"].any(), "a quenched placement moved under a second quench"

    drv = mcq_amd.drivers.run_competition
    energy, heights, path, info = drv(N=12, n_runs=128, n_steps=77, out_dir=str(tmp_path), timestamp="t", heatbath_sweeps=30, quench=True, **kw)
    r = int(np.argmin(res["quenched_energy"]))
    assert os.path.exists(path) and "quenched" in os.path.basename(path) and heights.shape == (12, 12)
    assert ru.recount("board", 12, heights.ravel()) == energy == int(res["quenched_energy"].min())
    assert info == {"quenched": True, "run": r, "energy_before": int(res["best_energy"][r]), "moves": int(res["quench_moves"][r])}
    np.testing.assert_array_equal(heights.ravel(), res["quenched_state"][r])
    # without the quench and without resampling: the board of the lowest best_energy, in the reference's format
    energy2, heights2, path2 = drv(N=12, n_runs=64, n_steps=77, out_dir=str(tmp_path), timestamp="u", heatbath_sweeps=20)
    solo = heatbath.anneal_heatbath(12, 20, "random", LIN, abi.seeds_for(42, 64))
    r2 = int(np.argmin(solo["best_energy"]))
    assert energy2 == int(solo["best_energy"][r2]) == ru.recount("board", 12, heights2.ravel())
    np.testing.assert_array_equal(heights2.ravel(), solo["best_state"][r2])
    written = np.loadtxt(path2, delimiter=",", dtype=np.int64)
    np.testing.assert_array_equal(written[:, 2], heights2.ravel())
    # without the argument the driver writes what it wrote before: the Metropolis chains' best board
    energy3, heights3, path3 = drv(N=12, n_runs=64, n_steps=3000, out_dir=str(tmp_path), timestamp="v")
    p = abi.make_params(12, 3000, "random", LIN, 64, mcmc_type="board")
    ref, _ = mcq_amd._lib.run_host(p, abi.seeds_for(42, 64), trace=False)
    r3 = int(np.argmin(ref["best_energy"]))
    assert energy3 == int(ref["best_energy"][r3]) and os.path.basename(path3) == "best_heights_12_v.txt"
    np.testing.assert_array_equal(heights3.ravel(), ref["best_state"][r3])


def test_torch_tensors_on_a_side_stream_in_a_fresh_process(tmp_path):
    """heatbath_device on a non-default stream with no synchronise inside: the call returns while a long kernel queued before it on the
    same stream still holds the stream, and the results are right once the stream is waited for."""
    out = str(tmp_path / "h.npz")
    code = f"""
import sys, numpy as np
sys.path.insert(0, {ROOT!r})
import torch, mcq_amd
from tests import quench_util as qu
dev = torch.device("cuda", 0)
s = qu.random_boards(12, 4099, 77, over=True)
seeds = mcq_amd.abi.seeds_for(9, 4099)
betas = [1.0, 2.0, 3.0]
side = torch.cuda.Stream(dev)
t = torch.from_numpy(s).to(dev)
dseeds = torch.from_numpy(seeds.view(np.int32)).to(dev)
dtab = mcq_amd.heatbath.device_table(betas, dev)
mcq_amd.heatbath.heatbath_device(12, t[:8].contiguous(), seeds[:8], betas)  # the first launch loads the library's code object: not part of what is shown
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
    res = mcq_amd.heatbath.heatbath_device(12, t, dseeds, dtab, first_sweep=3, trace=True)  # (stream=None: torch's current stream, which is `side`)
    pending = not side.query()
torch.cuda.Stream.synchronize, torch.cuda.synchronize = real, real_all
side.synchronize()
got = mcq_amd.heatbath.to_numpy(res)
np.savez({out!r}, pending=pending, n_syncs=len(syncs), inp=s, seeds=seeds, **got)
"""
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT, timeout=600)
    with np.load(out) as z:
        assert int(z["n_syncs"]) == 0, "heatbath_device synchronised"
        assert bool(z["pending"]), "the stream had drained before heatbath_device returned: the call cannot be shown to be asynchronous"
        want = heatbath.heatbath_states_host(12, z["inp"], z["seeds"], [1.0, 2.0, 3.0], first_sweep=3, trace=True)
        hu.assert_equal({k: z[k] for k in hu.FIELDS + ("energy_hist",)}, want, "side stream, fresh process", hist=True)
