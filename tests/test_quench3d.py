"""GPU: the full_3d quench kernel (mcq_quench3d_device) against the library's host code (mcq_quench3d_host) bit for bit on every
output, as the device recount of what real full_3d sweeps accumulated, and on torch tensors on a stream of its own."""
import os
import subprocess
import sys

import numpy as np
import pytest

import mcq_amd
from tests import quench3d_util as qu

abi = mcq_amd.abi
quench = mcq_amd.quench
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIN = {"type": "linear_annealing", "beta_start": 1.0, "beta_end": 3.0}

# the three instantiations -- 64 lanes and a byte field (N <= 12), 256 lanes and a byte field (N <= 19), 1 024 lanes and a 16-bit
# field (N <= 32) -- at both ends of each: (N, Q or None = N^2)
SIZES = ((2, None), (3, None), (5, None), (8, None), (12, None), (13, None), (16, None), (19, None), (20, None), (24, 300), (32, 200), (32, None))


def _placements(N, n, seed, Q=None):
    Qn = N * N if Q is None else Q
    s = qu.random_placements(N, n, seed, Q=Q, over=seed % 2 == 1).reshape(n, Qn, 3)
    if n > 2:
        s[1, Qn - 1] = s[1, 0]  # a repeated cell
    if n > 4:
        s[3] = 255  # every byte clamped: all queens in one cell
    return s.reshape(n, 3 * Qn)


@pytest.mark.parametrize("N,Q", SIZES)
def test_kernel_equals_the_host_code(N, Q):
    counts = (1, 3, 5, 17) if N <= 13 else (1, 3, 5) if N <= 20 else (1, 3)
    for idx, n in enumerate(counts):
        for mp in (0, 1, 2) if idx < 2 else (0,):
            s = _placements(N, n, 100 * N + idx, Q=Q)
            want = quench.quench_queens_host(N, s, Q=Q, max_passes=mp)
            got = quench.quench_queens(N, s, Q=Q, max_passes=mp)
            qu.assert_equal(got, want, f"N={N} Q={Q}, {n} chains, max_passes={mp}")
            for k in qu.FIELDS:
                assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
    # against the restatement too, where it is quick
    if N <= 13:
        s = _placements(N, 3, 5 * N, Q=Q)
        qu.assert_equal(quench.quench_queens(N, s, Q=Q), qu.quench_many(N, s, Q=Q), f"N={N} vs the restatement")


def test_other_queen_counts():
    """Q != N^2: two queens, one free cell, in between; on every instantiation."""
    for idx, (N, Q, n) in enumerate(((2, 2, 5), (2, 7, 5), (3, 26, 5), (5, 124, 3), (6, 20, 7), (6, 100, 7), (12, 60, 7), (12, 300, 5), (12, 1727, 2),
                                     (13, 2, 3), (17, 100, 5), (19, 1000, 2), (19, 6858, 1), (20, 2, 3), (24, 1000, 2), (32, 3000, 1))):
        s = _placements(N, n, 900 + idx, Q=Q)
        for mp in (0, 1):
            want = quench.quench_queens_host(N, s, Q=Q, max_passes=mp)
            got = quench.quench_queens(N, s, Q=Q, max_passes=mp)
            qu.assert_equal(got, want, f"N={N} Q={Q} max_passes={mp}")


def test_ragged_and_large_chain_counts():
    """One chain per workgroup: counts around the wavefront and workgroup sizes, and the 65 536 chains of the flagship shape."""
    for N, Q, n in ((12, None, 63), (12, None, 65), (8, None, 1025), (16, None, 257), (24, 200, 33), (12, None, 65536)):
        s = _placements(N, n, N + n, Q=Q)
        want = quench.quench_queens_host(N, s, Q=Q)
        got = quench.quench_queens(N, s, Q=Q)
        qu.assert_equal(got, want, f"N={N}, {n} chains")
        assert (got["conflicts"].sum(axis=1) == 2 * got["energy_out"]).all()
        ok = got["flags"] == 0
        assert (got["n_passes"][ok] <= got["energy_in"][ok] + 1).all() and (got["n_passes"][ok] >= 1).all()
        assert (got["n_passes"][~ok] == 0).all() and int((~ok).sum()) == (2 if n > 4 else 1 if n > 2 else 0)


def test_in_place_and_optional_outputs():
    import torch

    dev = torch.device("cuda", torch.cuda.current_device())
    st = torch.cuda.current_stream(dev)
    for N, Q, n, mp in ((12, None, 37, 0), (16, 100, 9, 1), (24, 150, 3, 2)):
        Qn = N * N if Q is None else Q
        s = _placements(N, n, 31 * N, Q=Q)
        want = quench.quench_queens_host(N, s, Q=Q, max_passes=mp)
        t = torch.from_numpy(s.reshape(n, Qn, 3)).to(dev)  # the [n][Q][3] form
        res = quench.quench_queens_device(N, t, Q=Q, max_passes=mp, out=t)  # in place
        st.synchronize()
        assert res["state"] is t and tuple(res["conflicts"].shape) == (n, Qn)
        qu.assert_equal(quench.to_numpy(res), want, f"N={N} in place")
        # only the placements: every per-chain output is optional
        q = abi.Quench3D()
        t2, o2 = torch.from_numpy(s).to(dev), torch.zeros((n, 3 * Qn), dtype=torch.uint8, device=dev)
        q.N, q.n_queens, q.n_chains, q.max_passes, q.state_in, q.state_out = N, Qn, n, mp, t2.data_ptr(), o2.data_ptr()
        mcq_amd._lib.quench3d_device(q, st)
        st.synchronize()
        np.testing.assert_array_equal(o2.cpu().numpy(), want["state"])
        np.testing.assert_array_equal(t2.cpu().numpy(), s)  # out of place: the input is untouched


@pytest.mark.parametrize("N", (8, 12, 16))
def test_energy_in_is_the_sweeps_own_energy(N):
    """The device recount of what the sweep accumulated step by step: best_state / final_state of real full_3d sweeps (the slim
    kernels at N = 8 and 12, the general one at 16)."""
    n = 256
    res, _ = mcq_amd.experiments.start_chains(N, 4000, "random", LIN, abi.seeds_for(42, n), mcmc_type="full_3d", trace=False, states=True)
    for which in ("best", "final"):
        got = quench.quench_queens(N, res[which + "_state"])
        np.testing.assert_array_equal(got["energy_in"], res[which + "_energy"], err_msg=f"N={N}: energy_in of {which}_state")
        assert (got["energy_out"] <= got["energy_in"]).all() and not got["flags"].any()
        qu.assert_equal(got, quench.quench_queens_host(N, res[which + "_state"]), f"N={N} {which}_state")
        print(f"N={N} {which}_state: min {int(got['energy_in'].min())} -> {int(got['energy_out'].min())}, "
              f"already local minima {int((got['n_moves'] == 0).sum())} of {n}")
        for r in (0, n // 2, n - 1):
            assert qu.pairwise_energy(N, got["state"][r]) == int(got["energy_out"][r])
        if N <= 12:
            assert qu.is_local_minimum(N, got["state"][0])


def test_torch_tensors_on_a_side_stream_in_a_fresh_process(tmp_path):
    """quench_queens_device on a non-default stream with no synchronise inside: the call returns while a long kernel queued before it
    on the same stream still holds the stream, and the results are right once the stream is waited for."""
    out = str(tmp_path / "q.npz")
    code = f"""
import sys, numpy as np
sys.path.insert(0, {ROOT!r})
import torch, mcq_amd
from tests import quench3d_util as qu
dev = torch.device("cuda", 0)
s = qu.random_placements(12, 4099, 77, over=True)
side = torch.cuda.Stream(dev)
t = torch.from_numpy(s).to(dev)
mcq_amd.quench.quench_queens_device(12, t[:8].contiguous())  # the first launch loads the library's code object: not part of what is shown
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
    res = mcq_amd.quench.quench_queens_device(12, t)  # (stream=None: torch's current stream, which is `side`)
    pending = not side.query()
torch.cuda.Stream.synchronize, torch.cuda.synchronize = real, real_all
side.synchronize()
got = mcq_amd.quench.to_numpy(res)
np.savez({out!r}, pending=pending, n_syncs=len(syncs), inp=s, **got)
"""
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT, timeout=600)
    with np.load(out) as z:
        assert int(z["n_syncs"]) == 0, "quench_queens_device synchronised"
        assert bool(z["pending"]), "the stream had drained before quench_queens_device returned: the call cannot be shown to be asynchronous"
        want = quench.quench_queens_host(12, z["inp"])
        qu.assert_equal({k: z[k] for k in qu.FIELDS}, want, "side stream, fresh process")
