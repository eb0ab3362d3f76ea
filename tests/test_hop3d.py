"""GPU: the basin-hopping kernel of full_3d placements (mcq_hop3d_device) against the library's host code (mcq_hop3d_host) bit for bit on
every output at both ends of every instantiation (W = 64 to N = 12, 256 to N = 19, 1024 beyond); a cut run, in place, only the
placements, a stream of its own, and the anneal_heatbath hook against the composed calls.  Before a group of comparisons counts, the
restatement (tests/hop3d_util.py) must say that it holds rejected hops, committed hops, an improving hop, a draw onto an occupied cell
and a queen drawn twice: otherwise the restore path, the commit path or the refused draw never ran.

Beyond the host code: the kernel against the full restatement at N = 3 and 4; the stream on both sides of word 2^35 and
kick = MCQ_MAX_HOP_KICK against the restated loop, whose words are Python integers; and at N = 13 and 20 state and best_state certified
as minima by NumPy (hop3d_util.is_local_minimum: quench3d_util's property from one attack matrix, held against it on the CPU) and
recounted pair by pair by tests/quench3d_util.py, not by kernels that share the code under test."""
import functools

import numpy as np
import pytest

import mcq_amd
from tests import hop3d_util as h3
from tests import quench3d_util as q3

abi = mcq_amd.abi
quench = mcq_amd.quench
pytestmark = pytest.mark.gpu

# the instantiations: both ends of each
GROUPS = {12: (2, 12), 19: (13, 19), 32: (20, 32)}
DEEP_FROM = 13  # from this N on a short run from a shallow start rejects nothing: most comparisons start from deepened minima
DEEP_HOPS = 150
DEEP_CHAINS = {13: 65, 19: 5, 20: 12}  # N = 32 starts shallow: its group's rejections come from N = 20, where a hop in four is rejected
TRACED = 12  # chains per comparison that the restated loop follows hop by hop


def _hops(N):
    return 12 if N <= 12 else 6 if N <= 19 else 3


def _cases(N):
    """(Q, chains, kick, slack, deep start) of the comparisons at N: every chain count up to N = 13 and few chains beyond, every kick and
    both slacks; Q = 2 and Q = N^3 - 1 at N = 4 (which rides in the first group) and N = 13."""
    if N == 4:
        return ((2, 5, 6, 0, False), (63, 5, 6, 0, False), (None, 5, 6, 0, False))
    if N < DEEP_FROM:
        return ((None, 1, 1, 0, False), (None, 5, 3, 2, False), (None, 65, N + 2, 0, False), (None, 5, N + 2, 2, False))
    if N == 13:
        return ((None, 65, N + 2, 0, True), (None, 5, 1, 2, True), (None, 5, 3, 0, True), (None, 1, N + 2, 2, False), (2, 5, 3, 0, False),
                (N ** 3 - 1, 1, 3, 2, False))
    if N == 32:  # Q = 1 024: 72 KiB of LDS, above what a kernel gets without the raised dynamic-LDS attribute
        return ((None, 1, N + 2, 0, False), (None, 2, 3, 2, False), (None, 1, 1, 0, False))
    return ((None, DEEP_CHAINS[N], N + 2, 0, True), (None, 5, 3, 0, True), (None, 1, 1, 2, True), (None, 1, N + 2, 2, False))


@functools.lru_cache(maxsize=None)
def _deep(N):
    """Placements of N >= DEEP_FROM behind DEEP_HOPS hops of the kernel itself with the large kick: inputs only -- whatever they are,
    host code and kernel must agree on them.  Coordinates N - 1 come as 255."""
    n = DEEP_CHAINS[N]
    s = quench.hop_queens(N, q3.random_placements(N, n, 100 * N), abi.seeds_for(900 + N, n), DEEP_HOPS, kick=N + 2)["state"]
    s[s == N - 1] = 255
    return s


def _start(N, Q, n, deep):
    return _deep(N)[DEEP_CHAINS[N] - n:].copy() if deep else q3.random_placements(N, n, 100 * N + n + (Q or 0), Q=Q, over=True)


@functools.lru_cache(maxsize=None)
def _reference(N, Q, n, kick, slack, deep):
    """(placements, seeds, host code's result) of one comparison, and the restatement's loop around the host descent next to it;
    computed once, shared and left unchanged."""
    s = _start(N, Q, n, deep)
    seeds = abi.seeds_for(500 + N, n)
    kw = dict(Q=Q, kick=kick, slack=slack)
    want = quench.hop_queens_host(N, s, seeds, _hops(N), hist=True, **kw)
    m = min(n, TRACED)
    traced = h3.hop_many(N, s[:m], seeds[:m], _hops(N), search="host", **kw)  # the traces of the first chains
    return s, seeds, want, traced


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_kernel_equals_the_host_code(group):
    import torch

    dev = torch.device("cuda", torch.cuda.current_device())
    sizes = GROUPS[group] + ((4,) if group == 12 else ())
    cov = h3.Coverage()
    for N in sizes:
        for Q, n, kick, slack, deep in _cases(N):
            s, seeds, want, traced = _reference(N, Q, n, kick, slack, deep)
            h3.assert_equal({k: v[: min(n, TRACED)] for k, v in want.items()}, traced, f"N={N} Q={Q}: host code vs the restated loop")
            cov.add(group, traced)
    print(group, cov.check(group))  # the condition on the inputs, before comparing
    for N in sizes:
        for Q, n, kick, slack, deep in _cases(N):
            s, seeds, want, _ = _reference(N, Q, n, kick, slack, deep)
            kw = dict(Q=Q, kick=kick, slack=slack)
            what = f"N={N} Q={Q}, {n} chains, kick={kick}, slack={slack}"
            got = quench.hop_queens(N, s, seeds, _hops(N), hist=True, **kw)
            h3.assert_equal(got, want, what)
            for k in quench.FIELDS_HOP3D:
                assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
            if N in (13, 20) and kick == 3 and Q is None:
                # state and best_state are minima by a certificate that owes nothing to the library, and so are their energies
                for k, e in (("state", "energy_out"), ("best_state", "best_energy")):
                    for r in (0, n - 1):
                        assert h3.is_local_minimum(N, got[k][r]), f"{what}: {k} of chain {r} is no minimum"
                        assert q3.pairwise_energy(N, got[k][r]) == int(got[e][r]), f"{what}: {k} of chain {r}"
            if n == 5 and Q is None:  # in place, and only the placements: every per-chain output is optional
                t, sd = torch.from_numpy(s).to(dev), torch.from_numpy(seeds.view(np.int32)).to(dev)
                res = quench.hop_queens_device(N, t, sd, _hops(N), out=t, **kw)
                torch.cuda.current_stream(dev).synchronize()
                assert res["state"] is t and "energy_hist" not in res
                h3.assert_equal(quench.to_numpy(res), want, what + ", in place", hist=False)
                q = abi.Hop3d()
                t2, o2 = torch.from_numpy(s).to(dev), torch.zeros_like(t)
                q.N, q.n_queens, q.n_chains, q.n_hops, q.kick, q.slack = N, 0, n, _hops(N), kick, slack
                q.seeds, q.state_in, q.state_out = sd.data_ptr(), t2.data_ptr(), o2.data_ptr()
                mcq_amd._lib.hop3d_device(q, torch.cuda.current_stream(dev))
                torch.cuda.current_stream(dev).synchronize()
                np.testing.assert_array_equal(o2.cpu().numpy(), want["state"])
                np.testing.assert_array_equal(t2.cpu().numpy(), s)  # out of place: the input is untouched


def test_kernel_equals_the_restatement_on_random_placements():
    for N, Q, n, hops, kick, slack in ((3, None, 6, 12, 3, 0), (4, None, 5, 12, 6, 0), (4, 30, 4, 10, 2, 1), (3, 26, 3, 8, 5, 2)):
        s = q3.random_placements(N, n, 300 + N + kick, Q=Q, over=True)
        seeds = abi.seeds_for(40 + N, n)
        want = h3.hop_many(N, s, seeds, hops, Q=Q, kick=kick, slack=slack)
        h3.assert_equal(quench.hop_queens(N, s, seeds, hops, Q=Q, kick=kick, slack=slack, hist=True), want, f"N={N} Q={Q} kick={kick}")


def test_a_repeated_placement_among_sound_ones():
    for N in (4, 13, 20):
        n, hops = 4, 3
        s = q3.random_placements(N, n, 20 + N, over=True)
        s[2, 3:6] = s[2, 0:3]  # queen 1 onto queen 0
        seeds = abi.seeds_for(8, n)
        want = quench.hop_queens_host(N, s, seeds, hops, kick=3, hist=True)
        np.testing.assert_array_equal(want["flags"], [0, 0, abi.HOP3D_REPEATED, 0])
        h3.assert_equal(quench.hop_queens(N, s, seeds, hops, kick=3, hist=True), want, f"N={N}: a repeat among sound placements")


def test_a_cut_run_is_the_unbroken_run():
    for N, Q, n, kick, slack in ((4, None, 5, 3, 1), (12, None, 3, 14, 0), (13, 100, 3, 5, 2)):
        s = q3.random_placements(N, n, 40 + N, Q=Q, over=True)
        seeds = abi.seeds_for(9, n)
        kw = dict(Q=Q, kick=kick, slack=slack, hist=True)
        whole = quench.hop_queens(N, s, seeds, 20, first_hop=4, **kw)
        parts, state, done = [], s, 4
        for hops in (7, 1, 12):
            parts.append(quench.hop_queens(N, state, seeds, hops, first_hop=done, **kw))
            state, done = parts[-1]["state"], done + hops
        h3.assert_equal(h3.merge(parts), whole, f"N={N}: 7 + 1 + 12 hops")
        h3.assert_equal(whole, quench.hop_queens_host(N, s, seeds, 20, first_hop=4, **kw), f"N={N}: the unbroken run")


@pytest.mark.parametrize("N,n,kick,how", ((4, 5, 3, "numpy"), (13, 2, 15, "host")))
def test_the_stream_beyond_word_2_34(N, n, kick, how):
    """Hops whose words lie on both sides of word 2^35, inside a kick, with an odd kick: the kernel against the restated loop, whose
    words are Python integers."""
    first, hops = h3.mark_first_hop(kick), 6
    assert h3.crosses_the_mark(kick, first, hops) and kick % 2 == 1 and (1 << 35) % (2 * kick) != 0
    s = q3.random_placements(N, n, 70 + N + kick, over=True)
    seeds = abi.seeds_for(11 + kick, n)
    kw = dict(kick=kick, slack=1, first_hop=first)
    want = h3.hop_many(N, s, seeds, hops, search=how, **kw)
    assert any(x in ("changed", "improved") for tr in want["trace"] for x in tr), "no hop past the mark changed a placement"
    h3.assert_equal(quench.hop_queens(N, s, seeds, hops, hist=True, **kw), want, f"N={N} kick={kick} first_hop={first}")


@pytest.mark.parametrize("N,n,hops", ((4, 3, 6), (12, 2, 4)))
def test_the_largest_kick(N, n, hops):
    """kick = MCQ_MAX_HOP_KICK: without slack a rejected hop restores nearly the whole placement, with a slack above every energy no
    hop is rejected -- by the restatement's traces."""
    s = q3.random_placements(N, n, 9 + N, over=True)
    seeds = abi.seeds_for(60 + N, n)
    rejected = 0
    for slack in (0, 13 * N ** 4):  # E <= 13 (N - 1) N^2 / 2
        want = h3.hop_many(N, s, seeds, hops, kick=abi.MAX_HOP_KICK, slack=slack, search="numpy" if N == 4 else "host")
        n_rej = sum(tr.count("rejected") for tr in want["trace"])
        assert want["drawn_twice"] == n * hops and want["occupied"] > 0 and (slack == 0 or n_rej == 0)
        rejected += n_rej
        got = quench.hop_queens(N, s, seeds, hops, kick=abi.MAX_HOP_KICK, slack=slack, hist=True)
        h3.assert_equal(got, want, f"N={N} kick={abi.MAX_HOP_KICK} slack={slack}")
        assert slack == 0 or (got["n_accepted"] == hops).all()
    assert rejected >= 1, "no hop was rejected without slack"


def test_torch_tensors_on_a_side_stream(monkeypatch):
    """hop_queens_device on a stream that is not the current one, with no synchronise inside."""
    import torch

    dev = torch.device("cuda", torch.cuda.current_device())
    N, n = 6, 257
    s = q3.random_placements(N, n, 77, over=True)
    seeds = abi.seeds_for(21, n)
    want = quench.hop_queens_host(N, s, seeds, 8, kick=3, slack=1, hist=True)
    side = torch.cuda.Stream(dev)
    t, sd = torch.from_numpy(s).to(dev), torch.from_numpy(seeds.view(np.int32)).to(dev)
    torch.cuda.synchronize()
    syncs = []
    real, real_all = torch.cuda.Stream.synchronize, torch.cuda.synchronize
    monkeypatch.setattr(torch.cuda.Stream, "synchronize", lambda self: (syncs.append("stream"), real(self))[1])
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: (syncs.append("device"), real_all(*a, **k))[1])
    res = quench.hop_queens_device(N, t.reshape(n, N * N, 3), sd, 8, kick=3, slack=1, hist=True, stream=side)
    with torch.cuda.stream(side):
        res2 = quench.hop_queens_device(N, res["state"], sd, 0)  # (stream=None: torch's current stream, `side`)
    assert syncs == [], "hop_queens_device synchronised"
    monkeypatch.undo()
    side.synchronize()
    assert tuple(res["state"].shape) == (n, N * N, 3)
    h3.assert_equal(quench.to_numpy(res), want, "side stream")
    got2 = quench.to_numpy(res2)
    np.testing.assert_array_equal(got2["state"].reshape(n, -1), want["state"])  # the output is a fixed point
    assert not got2["n_moves"].any() and (got2["n_passes"] == 1).all()
    np.testing.assert_array_equal(got2["energy_in"], want["energy_out"])
    with pytest.raises(ValueError, match="seeds"):
        quench.hop_queens_device(N, t, sd[:5], 1)
    with pytest.raises(ValueError, match="uint8 tensor"):
        quench.hop_queens_device(N, t.to(torch.int32), sd, 1)
    with pytest.raises(ValueError, match="bytes of LDS"):
        quench.hop_queens_device(32, torch.zeros((1, 3 * 23521), dtype=torch.uint8, device=dev), sd[:1], 1, Q=23521)


def test_the_annealing_hook_equals_the_composed_calls():
    heatbath = mcq_amd.heatbath
    N, n, lin = 6, 64, {"type": "linear_annealing", "beta_start": 1.0, "beta_end": 3.0}
    seeds = abi.seeds_for(42, n)
    base = heatbath.anneal_heatbath(N, 12, "random", lin, seeds, mcmc_type="full_3d")
    assert not any(k.startswith("hop") for k in base)  # hops=0: what it was
    res = heatbath.anneal_heatbath(N, 12, "random", lin, seeds, mcmc_type="full_3d", hops=20, hop_kick=3)
    for k in base:
        np.testing.assert_array_equal(res[k], base[k], err_msg=k)
    h = quench.hop_queens(N, base["best_state"], seeds, 20, kick=3)
    for k, f in (("hopped_state", "best_state"), ("hopped_energy", "best_energy"), ("hop_accepted", "n_accepted"), ("hop_improved", "n_improved"),
                 ("hop_best_hop", "best_hop")):
        np.testing.assert_array_equal(res[k], h[f], err_msg=k)
    assert (res["hopped_energy"] <= base["best_energy"]).all() and (res["hopped_energy"] < base["best_energy"]).any()
    for r in (0, n - 1):
        assert q3.pairwise_energy(N, res["hopped_state"][r]) == int(res["hopped_energy"][r])
    # behind the quench: the hops take the quenched placements
    both = heatbath.anneal_heatbath(N, 12, "random", lin, seeds, mcmc_type="full_3d", quench=True, hops=5)
    h2 = quench.hop_queens(N, both["quenched_state"], seeds, 5, kick=2)
    np.testing.assert_array_equal(both["hopped_state"], h2["best_state"])
    np.testing.assert_array_equal(both["hopped_energy"], h2["best_energy"])
    assert (h2["energy_start"] == both["quenched_energy"]).all()  # a quenched placement is a fixed point of L
