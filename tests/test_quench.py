"""GPU: the quench kernel (mcq_quench_device) against the library's host code (mcq_quench_host) bit for bit on every output, as the
device recount of what real sweeps accumulated, behind population annealing and the competition driver, and on torch tensors on a
stream of its own."""
import os
import subprocess
import sys

import numpy as np
import pytest

import mcq_amd
from tests import quench_util as qu
from tests import resume_util as ru

abi = mcq_amd.abi
quench = mcq_amd.quench
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIN = {"type": "linear_annealing", "beta_start": 1.0, "beta_end": 3.0}

# every group width (16, 32, 64 lanes) and two heights per lane (N > 64)
SIZES = (2, 3, 8, 12, 13, 16, 17, 24, 32, 33, 64, 65, 128)


def _boards(N, n, seed):
    s = qu.random_boards(N, n, seed, over=seed % 2 == 1)
    s[0] = seed % N  # all heights equal
    if n > 2:
        s[1] = 255  # clamped
    return s


@pytest.mark.parametrize("N", SIZES)
def test_kernel_equals_the_host_code(N):
    counts = (1, 3, 5, 17) if N <= 33 else (1, 3, 5) if N <= 65 else (1, 3)
    for idx, n in enumerate(counts):
        for mp in (0, 1, 2) if idx < 2 else (0,):
            s = _boards(N, n, 100 * N + idx)
            want = quench.quench_states_host(N, s, max_passes=mp)
            got = quench.quench_states(N, s, max_passes=mp)
            qu.assert_equal(got, want, f"N={N}, {n} chains, max_passes={mp}")
            for k in qu.FIELDS:
                assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
    # against the restatement too, where it is quick
    if N <= 17:
        s = _boards(N, 3, 5 * N)
        qu.assert_equal(quench.quench_states(N, s), qu.quench_many(N, s), f"N={N} vs the restatement")


def test_ragged_and_large_chain_counts():
    for N, n in ((12, 1025), (8, 1025), (24, 1025), (40, 257), (12, 65536)):
        s = _boards(N, n, N + n)
        want = quench.quench_states_host(N, s)
        got = quench.quench_states(N, s)
        qu.assert_equal(got, want, f"N={N}, {n} chains")
        assert (got["conflicts"].sum(axis=1) == 2 * got["energy_out"]).all()
        assert (got["n_passes"] <= got["energy_in"] + 1).all() and (got["n_passes"] >= 1).all()


def test_in_place_and_optional_outputs():
    import torch

    dev = torch.device("cuda", torch.cuda.current_device())
    st = torch.cuda.current_stream(dev)
    for N, n, mp in ((12, 37, 0), (20, 9, 1), (70, 3, 2)):
        s = _boards(N, n, 31 * N)
        want = quench.quench_states_host(N, s, max_passes=mp)
        t = torch.from_numpy(s).to(dev)
        res = quench.quench_device(N, t, max_passes=mp, out=t)  # in place
        st.synchronize()
        assert res["state"] is t
        qu.assert_equal(quench.to_numpy(res), want, f"N={N} in place")
        # only the placements: every per-chain output is optional
        q = abi.Quench()
        t2, o2 = torch.from_numpy(s).to(dev), torch.zeros((n, N * N), dtype=torch.uint8, device=dev)
        q.N, q.mode, q.n_chains, q.max_passes, q.state_in, q.state_out = N, abi.MODE_BOARD, n, mp, t2.data_ptr(), o2.data_ptr()
        mcq_amd._lib.quench_device(q, st)
        st.synchronize()
        np.testing.assert_array_equal(o2.cpu().numpy(), want["state"])
        np.testing.assert_array_equal(t2.cpu().numpy(), s)  # out of place: the input is untouched


@pytest.mark.parametrize("N", (6, 12, 24))
def test_energy_in_is_the_sweeps_own_energy(N):
    """The device recount of what the sweep accumulated step by step: best_state / final_state of real board sweeps."""
    n = 256
    p = abi.make_params(N, 4000, "random", LIN, n, mcmc_type="board")
    res, _ = mcq_amd._lib.run_host(p, abi.seeds_for(42, n), trace=False)
    for which in ("best", "final"):
        got = quench.quench_states(N, res[which + "_state"])
        np.testing.assert_array_equal(got["energy_in"], res[which + "_energy"], err_msg=f"N={N}: energy_in of {which}_state")
        assert (got["energy_out"] <= got["energy_in"]).all()
        print(f"N={N} {which}_state: min {int(got['energy_in'].min())} -> {int(got['energy_out'].min())}, "
              f"already local minima {int((got['n_moves'] == 0).sum())} of {n}")
        for r in (0, n // 2, n - 1):
            assert ru.recount("board", N, got["state"][r]) == int(got["energy_out"][r])
            assert qu.is_local_minimum(N, got["state"][r])


def test_population_annealing_with_quench(tmp_path):
    pop = mcq_amd.population
    kw = dict(population=128, resample_seed=1, mcmc_type="board")
    seeds = abi.seeds_for(42, 256)
    plain, lin0 = pop.anneal_population(12, 6000, "random", LIN, seeds, 500, **kw)
    res, lin1 = pop.anneal_population(12, 6000, "random", LIN, seeds, 500, quench=True, **kw)
    new = {"quenched_state", "quenched_energy", "quench_moves"}
    assert set(res) == set(plain) | new and not (new & set(plain))
    for k, v in plain.items():
        np.testing.assert_array_equal(res[k], v, err_msg=f"{k} changed with quench=True")
    for k, v in lin0.items():
        np.testing.assert_array_equal(np.asarray(lin1[k]), np.asarray(v), err_msg=f"lineage {k}")
    want = quench.quench_states(12, res["best_state"])
    np.testing.assert_array_equal(res["quenched_state"], want["state"])
    np.testing.assert_array_equal(res["quenched_energy"], want["energy_out"])
    np.testing.assert_array_equal(res["quench_moves"], want["n_moves"])
    np.testing.assert_array_equal(want["energy_in"], res["best_energy"])
    qu.assert_equal(want, quench.quench_states_host(12, res["best_state"]), "best_state of the population")

    # the competition driver: the board written is the lowest quenched energy over the runs
    out = mcq_amd.drivers.run_competition(N=12, n_runs=256, n_steps=6000, out_dir=str(tmp_path), timestamp="t", resample_every=500,
                                          population=128, resample_seed=1, quench=True)
    energy, heights, path, info = out
    assert os.path.exists(path) and "quenched" in os.path.basename(path) and heights.shape == (12, 12)
    assert ru.recount("board", 12, heights.ravel()) == energy == int(res["quenched_energy"].min())
    r = int(np.argmin(res["quenched_energy"]))
    assert info == {"quenched": True, "run": r, "energy_before": int(res["best_energy"][r]), "moves": int(res["quench_moves"][r])}
    np.testing.assert_array_equal(heights.ravel(), res["quenched_state"][r])
    written = np.loadtxt(path, delimiter=",", dtype=np.int64)
    np.testing.assert_array_equal(written[:, 2], heights.ravel())
    # ... and over independent chains (no resampling)
    energy2, heights2, path2, info2 = mcq_amd.drivers.run_competition(N=12, n_runs=64, n_steps=3000, out_dir=str(tmp_path), timestamp="u", quench=True)
    assert ru.recount("board", 12, heights2.ravel()) == energy2 <= info2["energy_before"] and info2["quenched"]
    plain3 = mcq_amd.drivers.run_competition(N=12, n_runs=64, n_steps=3000, out_dir=str(tmp_path), timestamp="v")
    assert len(plain3) == 3 and energy2 <= plain3[0]
    # run_population hands the same fields on
    tup = mcq_amd.experiments.run_population(12, 6000, "random", None, 256, 500, population=128, resample_seed=1, base_seed=42, schedule_params=LIN,
                                             mcmc_type="board", quench=True)
    assert len(tup) == 7 and tup[1] == [int(v) for v in res["best_energy"]]
    np.testing.assert_array_equal(tup[6]["quenched_energy"], res["quenched_energy"])


def test_torch_tensors_on_a_side_stream_in_a_fresh_process(tmp_path):
    """quench_device on a non-default stream with no synchronise inside: the call returns while a long kernel queued before it on the
    same stream still holds the stream, and the results are right once the stream is waited for."""
    out = str(tmp_path / "q.npz")
    code = f"""
import sys, numpy as np
sys.path.insert(0, {ROOT!r})
import torch, mcq_amd
from tests import quench_util as qu
dev = torch.device("cuda", 0)
s = qu.random_boards(12, 4099, 77, over=True)
side = torch.cuda.Stream(dev)
t = torch.from_numpy(s).to(dev)
mcq_amd.quench.quench_device(12, t[:8].contiguous())  # the first launch loads the library's code object: not part of what is shown
torch.cuda.synchronize()
syncs = []
real = torch.cuda.Stream.synchronize
torch.cuda.Stream.synchronize = lambda self: (syncs.append("stream"), real(self))[1]
real_all = torch.cuda.synchronize
torch.cuda.synchronize = lambda *a, **k: (syncs.append("device"), real_all(*a, **k))[1]
with torch.cuda.stream(side):
    big = torch.empty(1 << 28, dtype=torch.float32, device=dev)
    for _ in range(50):
        big.add_(1.0)  # ~ tens of milliseconds of work ahead of the quench on the side stream
    res = mcq_amd.quench.quench_device(12, t)  # (stream=None: torch's current stream, which is `side`)
    pending = not side.query()
torch.cuda.Stream.synchronize, torch.cuda.synchronize = real, real_all
side.synchronize()
got = mcq_amd.quench.to_numpy(res)
np.savez({out!r}, pending=pending, n_syncs=len(syncs), inp=s, **got)
"""
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT, timeout=600)
    with np.load(out) as z:
        assert int(z["n_syncs"]) == 0, "quench_device synchronised"
        assert bool(z["pending"]), "the stream had drained before quench_device returned: the call cannot be shown to be asynchronous"
        want = quench.quench_states_host(12, z["inp"])
        qu.assert_equal({k: z[k] for k in qu.FIELDS}, want, "side stream, fresh process")
