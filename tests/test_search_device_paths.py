"""GPU: the two device wrappers of quench.py that no other test calls with a stream of the caller's that is not torch's current one --
quench_device and quench_queens_device -- in place, with every optional output, against their host twins.  (The other six searches
have such a call in their own files: hop, tabu, relink, quench_pairs, hop3d, tabu3d.)"""
import numpy as np
import pytest

import mcq_amd
from tests import quench3d_util as q3
from tests import quench_util as qu

quench = mcq_amd.quench
pytestmark = pytest.mark.gpu


def _on_a_side_stream(call, s, want):
    import torch

    dev = torch.device("cuda", torch.cuda.current_device())
    side = torch.cuda.Stream(dev)
    t = torch.from_numpy(s).to(dev)
    side.wait_stream(torch.cuda.current_stream(dev))  # the upload ran on the current stream
    res = call(t, side)
    side.synchronize()
    assert res["state"] is t and list(res) == list(want)
    got = quench.to_numpy(res)
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)


def test_quench_device_in_place_on_a_stream_of_the_callers():
    N, n = 4, 3
    s = qu.random_boards(N, n, 7)
    want = quench.quench_states_host(N, s)
    assert (want["n_moves"] > 0).any() and want["conflicts"].shape == (n, N * N)
    _on_a_side_stream(lambda t, side: quench.quench_device(N, t, out=t, stream=side), s, want)


def test_quench_queens_device_in_place_on_a_stream_of_the_callers():
    N, Q, n = 3, 5, 3
    s = q3.random_placements(N, n, 7, Q=Q)
    want = quench.quench_queens_host(N, s, Q=Q)
    assert want["conflicts"].shape == (n, Q)
    _on_a_side_stream(lambda t, side: quench.quench_queens_device(N, t, Q=Q, out=t, stream=side), s, want)
