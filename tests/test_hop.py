"""GPU: the basin-hopping kernel (mcq_hop_device) against the library's host code (mcq_hop_host) bit for bit on every output at both ends
of every instantiation, for both local searches; a cut run, in place, a stream of its own, and the run_competition hook against the
composed calls.  Before a group of comparisons counts, the restatement (tests/hop_util.py) must say that it holds rejected hops,
committed hops, an improving hop and a kick that draws a column twice with different heights: otherwise the restore or the commit path
never ran, or the order of a kick's draws never showed.

Beyond the host code: the stream on both sides of word 2^35 and kick = MCQ_MAX_HOP_KICK against the restated loop, whose words are
Python integers; n_hops = 0 at any first_hop against the quench kernels; and at N = 17, 24, 25, 32 state and best_state certified as
minima by the NumPy table and the exhaustive pair scan of tests/quench_pairs_util.py, not by kernels that share the code under test."""
import functools
import os

import numpy as np
import pytest

import mcq_amd
from tests import hop_util as hu
from tests import quench_pairs_util as qp
from tests import quench_util as qu
from tests import resume_util as ru

abi = mcq_amd.abi
quench = mcq_amd.quench
pytestmark = pytest.mark.gpu
SEARCHES = ("single", "pairs")

# the instantiations are padded N = 4, 8, 12, 16, 24, 32: both ends of each
GROUPS = {4: (2, 4), 8: (5, 8), 12: (9, 12), 16: (13, 16), 24: (17, 24), 32: (25, 32)}


def _hops(N):
    return 12 if N <= 16 else 4 if N <= 24 else 3


DEEP_FROM = 17  # from this N on most comparisons start from minima that many hops have deepened
DEEP_HOPS = 300
TRACED = 32  # chains per comparison that the restated loop follows hop by hop


def _cases(N):
    """(chains, kick, slack, deep start) of the comparisons at N: every chain count, every kick and both slacks.  At the large N a short run
    from a shallow start rejects next to nothing -- the energy still falls with every hop --, so three of the four cases start deep, the
    rejections come from the large kick without slack, which therefore gets the 65 chains."""
    if N < DEEP_FROM:
        return ((1, 1, 0, False), (5, 3, 2, False), (65, N + 2, 0, False), (5, N + 2, 2, False))
    return ((65, N + 2, 0, True), (5, 1, 2, True), (5, 3, 2, True), (1, N + 2, 0, False))


def _boards(N, n, seed):
    """Up to N = 16, boards a few kicks away from a minimum, so that the host code's first descent is short: the heights (3 i + 5 j) mod N,
    which attack little, with one column in eight redrawn; beyond, random boards.  Bytes >= N among them."""
    if N >= DEEP_FROM:
        return qu.random_boards(N, n, seed, over=True)
    rs = np.random.RandomState(seed)
    s = np.tile(qu.klarner(N), (n, 1))
    m = rs.random_sample(s.shape) < 0.125
    s[m] = rs.randint(0, N, size=int(m.sum())).astype(np.uint8)
    s[rs.random_sample(s.shape) < 0.02] = 255  # clamped
    return s


@functools.lru_cache(maxsize=None)
def _deep(N):
    """65 boards of N >= DEEP_FROM behind DEEP_HOPS hops of the kernel itself with the large kick: inputs only -- whatever they are, host
    code and kernel must agree on them.  Heights N - 1 come as 255."""
    s = quench.hop_states(N, _boards(N, 65, 100 * N), abi.seeds_for(900 + N, 65), DEEP_HOPS, kick=N + 2, local_search="pairs")["state"]
    s[s == N - 1] = 255
    return s


def _start(N, n, deep):
    return _deep(N)[65 - n:].copy() if deep else _boards(N, n, 100 * N + n)


@functools.lru_cache(maxsize=None)
def _reference(N, search, n, kick, slack, deep):
    """(boards, seeds, host code's result) of one comparison, and the restatement's loop around the host local search next to it; computed
    once, shared and left unchanged."""
    s = _start(N, n, deep)
    seeds = abi.seeds_for(500 + N, n)
    kw = dict(kick=kick, slack=slack, local_search=search)
    want = quench.hop_host(N, s, seeds, _hops(N), hist=True, **kw)
    traced = hu.hop_many(N, s[: min(n, TRACED)], seeds[: min(n, TRACED)], _hops(N), search="host", **kw)  # the traces of the first chains
    return s, seeds, want, traced


@pytest.mark.parametrize("search", SEARCHES)
@pytest.mark.parametrize("NP", sorted(GROUPS))
def test_kernel_equals_the_host_code(NP, search):
    import torch

    dev = torch.device("cuda", torch.cuda.current_device())
    cov = hu.Coverage()
    for N in GROUPS[NP]:
        for n, kick, slack, deep in _cases(N):
            s, seeds, want, traced = _reference(N, search, n, kick, slack, deep)
            hu.assert_equal({k: v[: min(n, TRACED)] for k, v in want.items()}, traced, f"N={N} {search}: host code vs the restated loop")
            cov.add(NP, traced)
    print(NP, search, cov.check(NP))  # the condition on the inputs, before comparing
    for N in GROUPS[NP]:
        for n, kick, slack, deep in _cases(N):
            s, seeds, want, _ = _reference(N, search, n, kick, slack, deep)
            kw = dict(kick=kick, slack=slack, local_search=search)
            what = f"N={N} {search}, {n} chains, kick={kick}, slack={slack}"
            got = quench.hop_states(N, s, seeds, _hops(N), hist=True, **kw)
            hu.assert_equal(got, want, what)
            for k in quench.FIELDS_HOP:
                assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
            if n == 5:  # in place, and only the placements: every per-chain output is optional
                t, sd = torch.from_numpy(s).to(dev), torch.from_numpy(seeds.view(np.int32)).to(dev)
                res = quench.hop_device(N, t, sd, _hops(N), out=t, **kw)
                torch.cuda.current_stream(dev).synchronize()
                assert res["state"] is t and "energy_hist" not in res
                hu.assert_equal(quench.to_numpy(res), want, what + ", in place", hist=False)
                q = abi.Hop()
                t2, o2 = torch.from_numpy(s).to(dev), torch.zeros((n, N * N), dtype=torch.uint8, device=dev)
                q.N, q.mode, q.n_chains, q.n_hops, q.kick, q.slack, q.local_search = N, abi.MODE_BOARD, n, _hops(N), kick, slack, abi.HOP_LOCAL_SEARCH[search]
                q.seeds, q.state_in, q.state_out = sd.data_ptr(), t2.data_ptr(), o2.data_ptr()
                mcq_amd._lib.hop_device(q, torch.cuda.current_stream(dev))
                torch.cuda.current_stream(dev).synchronize()
                np.testing.assert_array_equal(o2.cpu().numpy(), want["state"])
                np.testing.assert_array_equal(t2.cpu().numpy(), s)  # out of place: the input is untouched
            if n == 5 and kick == 3 and N >= DEEP_FROM:
                # state and best_state are minima by a certificate that owes nothing to the library: the NumPy table for single moves and,
                # under "pairs", the exhaustive scan of every aligned pair
                for k in ("state", "best_state"):
                    for r in (0, 4):
                        if search == "pairs":
                            qp.certify(N, got[k][r], f"{what}: {k} of chain {r}")
                        else:
                            assert qu.is_local_minimum(N, got[k][r]), f"{what}: {k} of chain {r} is no single-move minimum"
                        assert qu.energy(N, got[k][r]) == int(got["best_energy" if k == "best_state" else "energy_out"][r])


@pytest.mark.parametrize("search", SEARCHES)
def test_kernel_equals_the_restatement_on_random_boards(search):
    """Against the NumPy restatement itself, local search included, where it is quick; random boards, so the first descent is long."""
    for N, n, kick, slack in ((3, 4, 2, 0), (4, 3, 6, 1), (6, 2, 8, 0)):
        s = qu.random_boards(N, n, 7 * N, over=True)
        seeds = abi.seeds_for(3, n)
        want = hu.hop_many(N, s, seeds, 10, kick=kick, slack=slack, local_search=search)
        hu.assert_equal(quench.hop_states(N, s, seeds, 10, kick=kick, slack=slack, local_search=search, hist=True), want, f"N={N} {search} vs the restatement")


@pytest.mark.parametrize("search", SEARCHES)
def test_a_cut_run_is_the_unbroken_run(search):
    for N, n, kick, slack in ((12, 65, 3, 1), (15, 5, 17, 0)):
        s = qu.random_boards(N, n, 40 + N, over=True)
        seeds = abi.seeds_for(9, n)
        kw = dict(kick=kick, slack=slack, local_search=search, hist=True)
        whole = quench.hop_states(N, s, seeds, 30, first_hop=4, **kw)
        hu.assert_equal(whole, quench.hop_host(N, s, seeds, 30, first_hop=4, **kw), f"N={N} {search}: 30 hops")
        parts, state, done = [], s, 4
        for hops in (7, 1, 22):
            parts.append(quench.hop_states(N, state, seeds, hops, first_hop=done, **kw))
            state, done = parts[-1]["state"], done + hops
        hu.assert_equal(hu.merge(parts), whole, f"N={N} {search}: 7 + 1 + 22 hops")
        for p in parts[1:]:
            np.testing.assert_array_equal(p["energy_in"], p["energy_start"])
        # the outputs are fixed points of L, by the quench kernels
        for k in ("state", "best_state"):
            q = quench.quench_pairs(N, whole[k]) if search == "pairs" else quench.quench_states(N, whole[k])
            assert not q["n_moves"].any() and (search == "single" or ((q["certified"] == 1).all() and not q["n_pair_moves"].any())), k
            np.testing.assert_array_equal(q["energy_in"], whole["best_energy" if k == "best_state" else "energy_out"])
        hist = whole["energy_hist"].astype(np.int64)
        assert (np.diff(hist, axis=1) <= slack).all()
        np.testing.assert_array_equal(whole["best_energy"], hist.min(axis=1))
        np.testing.assert_array_equal(whole["best_hop"], hist.argmin(axis=1))


def _near_minima(N, n):
    """Boards whose local search is short at every N: those of _boards up to N = 16, minima with columns redrawn beyond."""
    return _boards(N, n, 30 + N) if N < DEEP_FROM else qp.kicked_minima(N, n, 4, 12)


@pytest.mark.parametrize("search", SEARCHES)
@pytest.mark.parametrize("N,n", ((8, 65), (16, 5), (32, 2)))
def test_the_stream_beyond_word_2_34(N, n, search):
    """Hops on both sides of word 2^35 of the stream, where the second counter word of a block goes from 1 to 2 -- inside a kick, with
    the odd kick --: the kernel against the host code, and against the restated loop (whose words are Python integers) on the first
    chains; then a run cut 7 + 1 + rest across the mark."""
    s = _near_minima(N, n)
    seeds = abi.seeds_for(700 + N, n)
    for kick, slack in ((3, 1), (N + 2, 0)):
        first, hops = hu.mark_first_hop(kick), 6
        assert hu.crosses_the_mark(kick, first, hops)
        kw = dict(kick=kick, slack=slack, local_search=search, first_hop=first)
        what = f"N={N} {search} kick={kick} first_hop={first}"
        got = quench.hop_states(N, s, seeds, hops, hist=True, **kw)
        hu.assert_equal(got, quench.hop_host(N, s, seeds, hops, hist=True, **kw), what)
        m = min(n, 3)
        traced = hu.hop_many(N, s[:m], seeds[:m], hops, search="host", **kw)
        hu.assert_equal({k: v[:m] for k, v in got.items()}, traced, what + ": kernel vs the restated loop")
        assert any(x in ("changed", "improved") for tr in traced["trace"] for x in tr), what
    kick = 3
    first = hu.mark_first_hop(kick, before=7)  # the kick of the single hop in the middle holds word 2^35
    assert hu.crosses_the_mark(kick, first + 7, 1)
    kw = dict(kick=kick, slack=1, local_search=search, hist=True)
    whole = quench.hop_states(N, s, seeds, 14, first_hop=first, **kw)
    parts, state, done = [], s, first
    for hops in (7, 1, 6):
        parts.append(quench.hop_states(N, state, seeds, hops, first_hop=done, **kw))
        state, done = parts[-1]["state"], done + hops
    hu.assert_equal(hu.merge(parts), whole, f"N={N} {search}: 7 + 1 + 6 hops across word 2^35")
    hu.assert_equal(whole, quench.hop_host(N, s, seeds, 14, first_hop=first, **kw), f"N={N} {search}: 14 hops across word 2^35")


@pytest.mark.parametrize("N,n,hops,searches", hu.MAX_KICK_CASES)
def test_the_largest_kick(N, n, hops, searches):
    """kick = MCQ_MAX_HOP_KICK: the kernel against the restated loop and the host code, without slack (rejections: the whole board is
    restored) and with a slack above every energy (none)."""
    rejected = 0
    for search in searches:
        for accept_all in (False, True):
            s, seeds, _, slack, want = hu.max_kick_case(N, search, accept_all)
            n_rej = sum(tr.count("rejected") for tr in want["trace"])
            assert n_rej == 0 or not accept_all
            rejected += n_rej
            kw = dict(kick=hu.MAX_KICK, slack=slack, local_search=search, hist=True)
            got = quench.hop_states(N, s, seeds, hops, **kw)
            hu.assert_equal(got, want, f"N={N} {search} kick={hu.MAX_KICK} slack={slack}: kernel vs the restated loop")
            if N < 32:  # (at N = 32 tests/test_hop_host.py holds host code = restated loop on these very inputs)
                hu.assert_equal(got, quench.hop_host(N, s, seeds, hops, **kw), f"N={N} {search} kick={hu.MAX_KICK} slack={slack}")
    assert rejected >= 2


@pytest.mark.parametrize("search", SEARCHES)
def test_no_hops_is_the_quench_at_any_first_hop(search):
    """n_hops = 0 is the local search alone, whatever first_hop and kick say: the quench kernels' and the host code's figures."""
    for N, n in ((6, 65), (12, 5), (17, 3), (32, 2)):
        s = _near_minima(N, n)
        seeds = abi.seeds_for(1, n)
        if search == "pairs":
            q, qh = quench.quench_pairs(N, s), quench.quench_pairs_host(N, s)
        else:
            q, qh = quench.quench_states(N, s), quench.quench_states_host(N, s)
        for first_hop, kick in ((0, 2), (hu.mark_first_hop(5), 5), ((1 << 52) - 1, 1024)):
            got = quench.hop_states(N, s, seeds, 0, kick=kick, first_hop=first_hop, local_search=search, hist=True)
            hu.assert_equal(got, quench.hop_host(N, s, seeds, 0, kick=kick, first_hop=first_hop, local_search=search, hist=True), f"N={N} {search}")
            for ref in (q, qh):
                for k in ("state", "energy_in", "energy_out", "n_moves") + (("n_pair_moves",) if search == "pairs" else ()):
                    np.testing.assert_array_equal(got[k], ref[k], err_msg=f"N={N} {search} first_hop={first_hop}: {k}")
                np.testing.assert_array_equal(got["best_state"], ref["state"])
                for k in ("energy_start", "best_energy"):
                    np.testing.assert_array_equal(got[k], ref["energy_out"], err_msg=k)
            np.testing.assert_array_equal(got["energy_hist"], q["energy_out"][:, None])
            assert not got["best_hop"].any() and not got["n_accepted"].any() and not got["n_improved"].any()
            assert search == "pairs" or not got["n_pair_moves"].any()


def test_torch_tensors_on_a_side_stream(monkeypatch):
    """hop_device on a stream that is not the current one, with no synchronise inside."""
    import torch

    dev = torch.device("cuda", torch.cuda.current_device())
    N, n = 12, 257
    s = _boards(N, n, 77)
    seeds = abi.seeds_for(21, n)
    want = quench.hop_host(N, s, seeds, 8, kick=3, slack=1, hist=True)
    side = torch.cuda.Stream(dev)
    t, sd = torch.from_numpy(s).to(dev), torch.from_numpy(seeds.view(np.int32)).to(dev)
    torch.cuda.synchronize()
    syncs = []
    real, real_all = torch.cuda.Stream.synchronize, torch.cuda.synchronize
    monkeypatch.setattr(torch.cuda.Stream, "synchronize", lambda self: (syncs.append("stream"), real(self))[1])
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: (syncs.append("device"), real_all(*a, **k))[1])
    res = quench.hop_device(N, t, sd, 8, kick=3, slack=1, hist=True, stream=side)
    with torch.cuda.stream(side):
        res2 = quench.hop_device(N, res["state"], sd, 0)  # (stream=None: torch's current stream, `side`)
    assert syncs == [], "hop_device synchronised"
    monkeypatch.undo()
    side.synchronize()
    hu.assert_equal(quench.to_numpy(res), want, "side stream")
    got2 = quench.to_numpy(res2)
    np.testing.assert_array_equal(got2["state"], want["state"])  # the output is a fixed point
    assert not got2["n_moves"].any() and not got2["n_pair_moves"].any()
    np.testing.assert_array_equal(got2["energy_in"], want["energy_out"])
    with pytest.raises(ValueError, match="seeds"):
        quench.hop_device(N, t, sd[:5], 1)
    with pytest.raises(ValueError, match="uint8 tensor"):
        quench.hop_device(N, t.to(torch.int32), sd, 1)


def test_the_competition_hook_equals_the_composed_calls(tmp_path):
    kw = dict(N=8, n_runs=64, n_steps=2000, base_seed=7, out_dir=str(tmp_path))
    e0, h0, p0 = mcq_amd.drivers.run_competition(timestamp="a", **kw)
    assert os.path.basename(p0) == "best_heights_8_a.txt"  # hops=0: what it was
    e1, h1, p1, info = mcq_amd.drivers.run_competition(timestamp="b", hops=20, hop_kick=3, **kw)
    # the composed calls: the same search, then hop_states on its best_state
    res, _ = mcq_amd.experiments.run_chains(8, 2000, "random", {"type": "linear_annealing", "beta_start": 1.0, "beta_end": 3.0}, abi.seeds_for(7, 64),
                                mcmc_type="board", early_stop_patience=None, trace=False, states=True)
    assert int(res["best_energy"].min()) == e0
    h = quench.hop_states(8, res["best_state"], abi.seeds_for(7, 64), 20, kick=3)
    r = int(np.argmin(h["best_energy"]))
    assert os.path.basename(p1) == "best_heights_8_b_hopped.txt" and os.path.exists(p1)
    assert e1 == int(h["best_energy"][r]) == ru.recount("board", 8, h1.ravel()) and e1 <= e0
    np.testing.assert_array_equal(h1.ravel(), h["best_state"][r])
    assert info == {"hopped": 20, "kick": 3, "run": r, "energy_before": int(res["best_energy"][r]), "energy_start": int(h["energy_start"][r]),
                    "accepted": int(h["n_accepted"][r]), "improved": int(h["n_improved"][r]), "best_hop": int(h["best_hop"][r])}
    # behind the heat bath with the pair-move quench: both suffixes
    e2, h2, p2, info2 = mcq_amd.drivers.run_competition(timestamp="c", heatbath_sweeps=12, quench="pairs", hops=5, **kw)
    assert os.path.basename(p2) == "best_heights_8_c_quenched_pairs_hopped.txt" and info2["quenched"] == "pairs" and info2["kick"] == 2
    assert ru.recount("board", 8, h2.ravel()) == e2 <= info2["energy_start"] <= info2["energy_before"]
