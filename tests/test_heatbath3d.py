"""GPU: the full_3d heat-bath kernel (mcq_heatbath3d_device) against the library's host code (mcq_heatbath3d_host) bit for bit on every
output, at both ends of its three instantiations, with winners in every lane's run, on ragged and large chain counts, in segments, in
place, on a stream of its own, and under anneal_heatbath(mcmc_type="full_3d")."""
import os
import subprocess
import sys

import numpy as np
import pytest

import mcq_amd
from tests import heatbath3d_util as h3
from tests import heatbath_util as hu
from tests import population_util as pu
from tests import quench3d_util as q3
from tests import quench_util as qu

abi = mcq_amd.abi
heatbath = mcq_amd.heatbath
quench = mcq_amd.quench
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIN = {"type": "linear_annealing", "beta_start": 1.0, "beta_end": 3.0}
BETAS = [0.0, 0.7, 3.0]

# the three instantiations -- 64 lanes and a byte field (N <= 12), 256 lanes and a byte field (N <= 19), 1 024 lanes and a 16-bit
# field (N <= 32) -- at both ends of each: (N, Q or None = N^2)
SIZES = ((2, None), (3, None), (5, None), (8, None), (12, None), (13, None), (16, None), (19, None), (20, None), (24, 300), (32, 200), (32, None))


def _placements(N, n, seed, Q=None):
    """As tests/test_quench3d.py builds them: one repeated placement and one all-255 placement among the chains."""
    Qn = N * N if Q is None else Q
    s = q3.random_placements(N, n, seed, Q=Q, over=seed % 2 == 1).reshape(n, Qn, 3)
    if n > 2:
        s[1, Qn - 1] = s[1, 0]  # a repeated cell
    if n > 4:
        s[3] = 255  # every byte clamped: all queens in one cell
    return s.reshape(n, 3 * Qn)


def _same(got, want, what, hist=True):
    h3.assert_equal(got, want, what, hist=hist)
    for k in h3.FIELDS + (("energy_hist",) if hist else ()):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)


@pytest.mark.parametrize("N,Q", SIZES)
def test_kernel_equals_the_host_code(N, Q):
    counts = (1, 3, 5, 17) if N <= 13 else (1, 3, 5) if N <= 20 else (1, 3)
    for idx, n in enumerate(counts):
        for n_sweeps in ((0, 1, 3) if idx < 2 else (3,)) if N < 24 else (1,):
            s = _placements(N, n, 100 * N + idx, Q=Q)
            seeds = abi.seeds_for(31 * N + idx, n)
            betas = (BETAS * 2)[idx % 3: idx % 3 + n_sweeps]  # every row leads once; N = 32 runs the beta = 0 row: W ~ 2^39
            first = (0, 5, (1 << 33) + 3)[idx % 3]
            want = heatbath.heatbath_queens_host(N, s, seeds, betas, Q=Q, first_sweep=first, trace=True)
            got = heatbath.heatbath_queens(N, s, seeds, betas, Q=Q, first_sweep=first, trace=True)
            _same(got, want, f"N={N} Q={Q}, {n} chains, betas={betas}")
            assert list(got["flags"]) == [int(r in (1, 3) and (r == 1 and n > 2 or r == 3 and n > 4)) for r in range(n)]
    if N <= 8:  # against the restatement too, where it is quick
        s = _placements(N, 3, 5 * N, Q=Q)
        seeds = abi.seeds_for(N, 3)
        h3.assert_equal(heatbath.heatbath_queens(N, s, seeds, BETAS, Q=Q, trace=True), h3.sweeps_many(N, s, seeds, BETAS, Q=Q), f"N={N} vs the restatement", hist=True)


def test_other_queen_counts():
    """Q != N^2: two queens, one free cell, in between; on every instantiation."""
    for idx, (N, Q, n) in enumerate(((2, 2, 5), (2, 7, 5), (3, 26, 5), (5, 124, 3), (12, 1727, 2), (13, 2, 3), (19, 1000, 2), (20, 2, 3), (32, 3000, 1))):
        s = _placements(N, n, 900 + idx, Q=Q)
        seeds = abi.seeds_for(idx, n)
        betas = [0.7, 0.0] if Q <= 124 else [0.7]
        want = heatbath.heatbath_queens_host(N, s, seeds, betas, Q=Q, trace=True)
        _same(heatbath.heatbath_queens(N, s, seeds, betas, Q=Q, trace=True), want, f"N={N} Q={Q}")


@pytest.mark.parametrize("N,n,n_sweeps", ((5, 1025, 2), (16, 257, 1)))
def test_selection_at_lane_edges(N, n, n_sweeps):
    """beta = 0: every free cell is as likely as any other, so over the chains the winners fall in every lane's run, first and last
    cells included."""
    s = q3.random_placements(N, n, 40 + N)
    seeds = abi.seeds_for(1234, n)
    want = heatbath.heatbath_queens_host(N, s, seeds, [0.0] * n_sweeps, trace=True)
    got = heatbath.heatbath_queens(N, s, seeds, [0.0] * n_sweeps, trace=True)
    _same(got, want, f"N={N}, {n} chains at beta = 0")
    z = got["state"].reshape(n, N * N, 3).astype(np.int64)
    hit = np.unique((z[:, :, 0] * N + z[:, :, 1]) * N + z[:, :, 2])
    assert len(hit) == N ** 3, "some cell of the cube was never drawn"


def test_ragged_and_large_chain_counts():
    for n in (63, 65):
        s = _placements(12, n, n)
        seeds = abi.seeds_for(n, n)
        _same(heatbath.heatbath_queens(12, s, seeds, [0.7, 3.0], trace=True), heatbath.heatbath_queens_host(12, s, seeds, [0.7, 3.0], trace=True), f"{n} chains")
    n = 65536
    s = np.tile(q3.random_placements(12, 256, 8), (n // 256, 1))
    got = heatbath.heatbath_queens(12, s, abi.seeds_for(5, n), [1.0])
    recount = quench.quench_queens(12, got["state"], max_passes=1, conflicts=False)
    np.testing.assert_array_equal(got["energy_out"], recount["energy_in"])
    np.testing.assert_array_equal(got["best_energy"], np.minimum(got["energy_in"], got["energy_out"]))
    assert not got["flags"].any() and not recount["flags"].any()
    np.testing.assert_array_equal(got["energy_in"], np.tile(got["energy_in"][:256], n // 256))
    assert len(np.unique(got["state"][::256], axis=0)) > 250  # one start placement, 256 seeds: 256 different chains


def test_device_segments_in_place_and_optional_outputs():
    import torch

    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev)
    for idx, (N, Q, n) in enumerate(((6, None, 9), (12, 100, 5), (16, None, 4), (24, 200, 2))):
        Qn = N * N if Q is None else Q
        s = _placements(N, n, 70 + idx, Q=Q)
        seeds = abi.seeds_for(3 + idx, n)
        betas = [0.3, 0.9, 1.5, 3.0]
        whole = heatbath.heatbath_queens_host(N, s, seeds, betas, Q=Q, first_sweep=2, trace=True)
        _same(heatbath.heatbath_queens(N, s, seeds, betas, Q=Q, first_sweep=2, trace=True), whole, f"N={N} whole")
        # two device segments with first_sweep carried over, the second in place, in the [n][Q][3] form, table and seeds on the device
        t = torch.from_numpy(s.reshape(n, Qn, 3)).to(dev)
        dtab = heatbath.device_table(betas, dev)
        dseeds = torch.from_numpy(seeds.view(np.int32).copy()).to(dev)
        a = heatbath.heatbath_queens_device(N, t, dseeds, dtab[:1], Q=Q, first_sweep=2)
        assert a["state"].shape == t.shape and a["state"].data_ptr() != t.data_ptr()
        b = heatbath.heatbath_queens_device(N, a["state"], dseeds, dtab[1:], Q=Q, first_sweep=3, out=a["state"], trace=True)
        st.synchronize()
        assert b["state"].data_ptr() == a["state"].data_ptr()
        got = heatbath.to_numpy(b)
        np.testing.assert_array_equal(got["state"].reshape(n, -1), whole["state"], err_msg=f"N={N}: segments, the second in place")
        np.testing.assert_array_equal(got["energy_out"], whole["energy_out"])
        np.testing.assert_array_equal(got["energy_hist"], whole["energy_hist"][:, 1:])
        np.testing.assert_array_equal(got["flags"], whole["flags"])
        np.testing.assert_array_equal(t.cpu().numpy().reshape(n, -1), s)  # out of place: the input is untouched
        # each optional output left out: the call with it alone, and the call with none
        tdt = {np.int32: torch.int32, np.int64: torch.int64}
        dt = heatbath.device_table(betas, dev)
        for only in tuple(abi.HEATBATH3D_DTYPES) + ("best_state", "energy_hist", None):
            t2, o2 = torch.from_numpy(s).to(dev), torch.zeros((n, 3 * Qn), dtype=torch.uint8, device=dev)
            q = abi.Heatbath3D()
            q.N, q.n_queens, q.n_chains, q.n_sweeps, q.first_sweep, q.table_len = N, Qn, n, len(betas), 2, dt.shape[1]
            q.seeds, q.table, q.state_in, q.state_out = dseeds.data_ptr(), dt.data_ptr(), t2.data_ptr(), o2.data_ptr()
            if only in abi.HEATBATH3D_DTYPES:
                buf = torch.zeros(n, dtype=tdt[abi.HEATBATH3D_DTYPES[only]], device=dev)
            elif only == "best_state":
                buf = torch.zeros((n, 3 * Qn), dtype=torch.uint8, device=dev)
            elif only == "energy_hist":
                buf = torch.zeros((n, len(betas) + 3), dtype=torch.int32, device=dev)  # a stride beyond n_sweeps + 1
                q.hist_stride = len(betas) + 3
            if only is not None:
                setattr(q, only, buf.data_ptr())
            mcq_amd._lib.heatbath3d_device(q, st)
            st.synchronize()
            np.testing.assert_array_equal(o2.cpu().numpy(), whole["state"], err_msg=f"N={N}: only {only}")
            if only == "energy_hist":
                np.testing.assert_array_equal(buf.cpu().numpy()[:, : len(betas) + 1], whole["energy_hist"])
                assert not buf.cpu().numpy()[:, len(betas) + 1:].any()
            elif only is not None:
                np.testing.assert_array_equal(buf.cpu().numpy(), whole[only], err_msg=f"N={N}: only {only}")
    with pytest.raises(ValueError, match="contiguous uint8 tensor on the GPU"):
        heatbath.heatbath_queens_device(6, torch.zeros((2, 108), dtype=torch.uint8), [1, 2], [1.0])
    with pytest.raises(ValueError, match="final_state layout of full_3d"):
        heatbath.heatbath_queens_device(6, torch.zeros((2, 107), dtype=torch.uint8, device=dev), [1, 2], [1.0])
    with pytest.raises(ValueError, match="n_chains"):
        heatbath.heatbath_queens(6, np.zeros((0, 108), dtype=np.uint8), [], [1.0])


def test_torch_tensors_on_a_side_stream_in_a_fresh_process(tmp_path):
    """heatbath_queens_device on a non-default stream with no synchronise inside: the call returns while work queued before it on the
    same stream still holds the stream, and the results are right once the stream is waited for."""
    out = str(tmp_path / "h.npz")
    code = f"""
import sys, numpy as np
sys.path.insert(0, {ROOT!r})
import torch, mcq_amd
from tests import quench3d_util as q3
dev = torch.device("cuda", 0)
n = 1031
s = q3.random_placements(8, n, 77, over=True)
seeds = mcq_amd.abi.seeds_for(9, n)
betas = [1.0, 2.0]
side = torch.cuda.Stream(dev)
t = torch.from_numpy(s).to(dev)
dseeds = torch.from_numpy(seeds.view(np.int32)).to(dev)
dtab = mcq_amd.heatbath.device_table(betas, dev)
mcq_amd.heatbath.heatbath_queens_device(8, t[:8].contiguous(), seeds[:8], betas)  # the first launch loads the library's code object
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
    res = mcq_amd.heatbath.heatbath_queens_device(8, t, dseeds, dtab, first_sweep=3, trace=True)  # (stream=None: torch's current stream, `side`)
    pending = not side.query()
torch.cuda.Stream.synchronize, torch.cuda.synchronize = real, real_all
side.synchronize()
got = mcq_amd.heatbath.to_numpy(res)
np.savez({out!r}, pending=pending, n_syncs=len(syncs), inp=s, seeds=seeds, **got)
"""
    subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-c", code], check=True, cwd=ROOT)
    with np.load(out) as z:
        assert int(z["n_syncs"]) == 0, "heatbath_queens_device synchronised"
        assert bool(z["pending"]), "the stream had drained before heatbath_queens_device returned: the call cannot be shown to be asynchronous"
        want = heatbath.heatbath_queens_host(8, z["inp"], z["seeds"], [1.0, 2.0], first_sweep=3, trace=True)
        h3.assert_equal({k: z[k] for k in h3.FIELDS + ("energy_hist",)}, want, "side stream, fresh process", hist=True)


def _as_call(res):
    return {"state": res["final_state"], "energy_in": res["initial_energy"], "energy_out": res["final_energy"], "best_energy": res["best_energy"],
            "best_sweep": res["best_sweep"], "best_state": res["best_state"], "n_changed": res["n_changed"], "flags": res["flags"],
            "energy_hist": res.get("energy_hist")}


def _compose_host(N, n_sweeps, start, sp, seeds, S, population, resample_seed):
    """The run anneal_heatbath(mcmc_type="full_3d") makes, composed on the host: heatbath_queens_host segments, population_util.plan in
    between, the fold of a segment's best values by a strictly lower energy."""
    n = len(seeds)
    R = n if population is None else population
    K = -(-n_sweeps // S)
    lengths = [S] * (K - 1) + [n_sweeps - (K - 1) * S]
    beta = abi.beta_values(sp, n_sweeps)
    offsets = np.random.RandomState(resample_seed).randint(0, 2**32, size=(K - 1, n // R), dtype=np.uint32)
    state, done, parents = start, 0, []
    hist = np.zeros((n, n_sweeps + 1), dtype=np.int32)
    for k, L in enumerate(lengths):
        seg = heatbath.heatbath_queens_host(N, state, seeds, beta[done: done + L], first_sweep=done, trace=True)
        if k == 0:
            best = {f: seg[f].copy() for f in ("best_energy", "best_sweep", "best_state", "n_changed")}
            first = seg
            hist[:, : L + 1] = seg["energy_hist"]
        else:
            lower = seg["best_energy"] < best["best_energy"]
            best["best_energy"][lower] = seg["best_energy"][lower]
            best["best_sweep"][lower] = seg["best_sweep"][lower] + done
            best["best_state"][lower] = seg["best_state"][lower]
            best["n_changed"] += seg["n_changed"]
            hist[:, done + 1: done + L + 1] = seg["energy_hist"][:, 1:]
        if k < K - 1:
            par, _ = pu.plan(seg["energy_out"], R, pu.table(beta[(k + 1) * S] - beta[k * S]), offsets[k])
            state = seg["state"][par]
            parents.append(par)
        done += L
    return dict(best, initial_energy=first["energy_in"], final_energy=seg["energy_out"], final_state=seg["state"], energy_hist=hist), np.array(parents)


def test_anneal_heatbath_full_3d():
    N, n, n_sweeps = 6, 64, 12
    seeds = abi.seeds_for(42, n)
    # without resampling: heatbath_queens_host on the start placements, which are the reference's own initial state of each chain
    plain = heatbath.anneal_heatbath(N, n_sweeps, "random", LIN, seeds, trace=True, mcmc_type="full_3d")
    zero = heatbath.anneal_heatbath(N, 0, "random", LIN, seeds, mcmc_type="full_3d")
    first, _ = mcq_amd._lib.run_host(abi.make_params(N, 1, "random", LIN, n, mcmc_type="full_3d"), seeds, trace=False)
    np.testing.assert_array_equal(zero["initial_energy"], first["initial_energy"])
    np.testing.assert_array_equal(zero["final_state"], zero["best_state"])
    assert zero["final_state"].shape == (n, 108) and not zero["flags"].any()
    want = heatbath.heatbath_queens_host(N, zero["final_state"], seeds, abi.beta_values(LIN, n_sweeps), trace=True)
    h3.assert_equal(_as_call(plain), want, "anneal_heatbath(full_3d) without resampling", hist=True)
    # given placements and another Q
    start = q3.random_placements(N, n, 9, Q=50)
    given = heatbath.anneal_heatbath(N, 5, start, LIN, seeds, mcmc_type="full_3d", Q=50)
    h3.assert_equal(_as_call(given), heatbath.heatbath_queens_host(N, start, seeds, abi.beta_values(LIN, 5), Q=50), "given placements, Q = 50")
    # resample_every = 4: the run composed on the host with the NumPy resampling plan
    got, lin = heatbath.anneal_heatbath(N, n_sweeps, "random", LIN, seeds, resample_every=4, population=32, resample_seed=3, trace=True, mcmc_type="full_3d")
    comp, parents = _compose_host(N, n_sweeps, zero["final_state"], LIN, seeds, 4, 32, 3)
    for k in ("initial_energy", "final_energy", "final_state", "best_energy", "best_sweep", "best_state", "n_changed", "energy_hist"):
        np.testing.assert_array_equal(got[k], comp[k], err_msg=f"resample_every=4: {k}")
    np.testing.assert_array_equal(lin["parents"], parents)
    assert lin["lengths"] == [4, 4, 4] and (lin["distinct_parents"] < 32).any(), "no boundary resampled anything"
    # quench=True: best_state through the full_3d quench
    res, _ = heatbath.anneal_heatbath(N, n_sweeps, "random", LIN, seeds, resample_every=4, population=32, resample_seed=3, quench=True, mcmc_type="full_3d")
    assert (res["quenched_energy"] <= res["best_energy"]).all()
    np.testing.assert_array_equal(res["best_state"], got["best_state"])
    wantq = quench.quench_queens_host(N, res["best_state"])
    np.testing.assert_array_equal(res["quenched_state"], wantq["state"])
    np.testing.assert_array_equal(res["quenched_energy"], wantq["energy_out"])
    np.testing.assert_array_equal(res["quench_moves"], wantq["n_moves"])
    # the board call with default keywords returns what it returned before
    boards = qu.random_boards(N, n, 4)
    board = heatbath.anneal_heatbath(N, 7, boards, LIN, seeds, trace=True)
    assert "flags" not in board
    hu.assert_equal({"state": board["final_state"], "energy_in": board["initial_energy"], "energy_out": board["final_energy"], "best_energy": board["best_energy"],
                     "best_sweep": board["best_sweep"], "best_state": board["best_state"], "n_changed": board["n_changed"], "energy_hist": board["energy_hist"]},
                    heatbath.heatbath_states_host(N, boards, seeds, abi.beta_values(LIN, 7), trace=True), "the board call", hist=True)
