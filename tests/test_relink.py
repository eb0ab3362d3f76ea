"""GPU: the path-relinking kernel (mcq_relink_device) against the library's host code (mcq_relink_host) bit for bit on every output and
dtype, the history included, under both local searches at both ends of every instantiation: 5 and 70 minima relinked with their
neighbour, and the calls of tests/relink_cases.py -- bytes >= N, d0 = 0, d0 = N^2 (1 024 steps at N = 32: the longest walk and every
value of rho), the window of candidates at its edges, max_steps below min_dist --, chain 0 of each against the restatement of
tests/relink_util.py; with and without the optional outputs; the largest fall and the largest rise of a step at N = 32; in place; a
stream of its own; the pool against its host form; and 4 096 heat-bath placements through the invariants of the rule, checked by the
quench kernels.  Before a comparison counts its coverage is asserted, from the restatement's traces and the host code's outputs; none
is computed from the kernel's outputs."""
import functools

import numpy as np
import pytest

import mcq_amd
from tests import relink_cases as rc
from tests import relink_util as ru

abi = mcq_amd.abi
quench = mcq_amd.quench
pytestmark = pytest.mark.gpu

# the instantiations are padded N = 4, 8, 12, 16, 24, 32: both ends of each
GROUPS = {4: (2, 4), 8: (5, 8), 12: (9, 12), 16: (13, 16), 24: (17, 24), 32: (25, 32)}
CHAINS = (5, 70)  # a handful of workgroups, and more than 64
LONG_WALKS_BELOW = 17  # up to N = 16 all 70 chains walk between distant minima


@functools.lru_cache(maxsize=None)
def _neighbours(N, n, search):
    """(minima, their neighbours as guides, seeds, min_dist, the host code's result): computed once, shared and left unchanged.  From
    N = 17 on the 70 chains are 14 copies of 5 pair-move minima, each with a seed and a guide of its own 8 columns away: a pair move costs
    the host code milliseconds there and a walk between two distant minima needs 60 of them per chain, which the 5 chains and the
    calls of tests/relink_cases.py pay; the 70 are there for the grid."""
    if n == 70 and N >= LONG_WALKS_BELOW:
        rs = np.random.RandomState(N)
        s = np.tile(quench.quench_pairs_host(N, ru.minima(N, 5, 300 + N), conflicts=False)["state"], (14, 1))
        g = s.copy()
        for r in range(n):
            cols = rs.choice(N * N, size=8, replace=False)
            g[r, cols] = (g[r, cols] + rs.randint(1, N, size=8)) % N
    else:
        s = ru.minima(N, n, 300 + N + n)
        g = ru.neighbours(s)
    s[s == N - 1] = 255  # clamped
    seeds = abi.seeds_for(400 + N, n)
    md = 1 if n == 5 else max(1, N * N // 8) if N < LONG_WALKS_BELOW else 2
    return s, g, seeds, md, quench.relink_host(N, s, g, seeds, min_dist=md, local_search=search, walk=n, hist=True)


def _assert_same(got, want, what):
    ru.assert_equal(got, want, what)
    for k in quench.FIELDS_RELINK:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k


@pytest.mark.parametrize("search", rc.SEARCHES)
@pytest.mark.parametrize("NP", sorted(GROUPS))
def test_kernel_equals_the_host_code(NP, search):
    import torch

    dev = torch.device("cuda", torch.cuda.current_device())
    cov = ru.Coverage()
    for N in GROUPS[NP]:
        for i, (name, s, g, seeds, kw, runs) in enumerate(rc.cases(N)):
            want = rc.hosted(N, i, search)
            cov.add_outputs(NP, ru.host_cover(N, want, g, kw["min_dist"]))
            # the host code's chain 0 is the restatement's.  Beyond N = 16 only the short walks and, at N = 32, the walk of d0 = 1 024 steps
            # are restated here (rc.cheap); tests/test_relink_host.py holds the host code to the restatement on chain 0 of every call at
            # every N, where the restatement's seconds per long walk cost no GPU time
            if runs and rc.cheap(N, name, kw):
                traced = rc.restated_chain0(N, i, search)
                ru.assert_equal(want, traced, f"N={N} {name} {search}: host code vs the restatement", rows=slice(0, 1))
                cov.add_traces(NP, traced["trace"])
        for n in CHAINS:
            s, g, seeds, md, want = _neighbours(N, n, search)
            cov.add_outputs(NP, ru.host_cover(N, want, g, md))
    print(NP, search, cov.check(NP, pairs=search == "pairs"))  # the condition on the inputs, before comparing
    for N in GROUPS[NP]:
        for i, (name, s, g, seeds, kw, runs) in enumerate(rc.cases(N)):
            got = quench.relink_states(N, s, g, seeds, local_search=search, hist=True, **kw)
            _assert_same(got, rc.hosted(N, i, search), f"N={N} {name} {search}")
            if name == "every column differs":
                assert (got["distance_in"] == N * N).all() and (got["n_steps"] == N * N).all()
        for n in CHAINS:
            s, g, seeds, md, want = _neighbours(N, n, search)
            what = f"N={N} {search}, {n} minima and their neighbours"
            _assert_same(quench.relink_states(N, s, g, seeds, min_dist=md, local_search=search, walk=n, hist=True), want, what)
            if n == 5:  # without the optional outputs, through the wrapper and on the bare block; in place
                slim = quench.relink_states(N, s, g, seeds, min_dist=md, local_search=search, walk=n, figures=False)
                assert set(slim) == {"state"}
                np.testing.assert_array_equal(slim["state"], want["state"])
                t, tg, sd = torch.from_numpy(s).to(dev), torch.from_numpy(g).to(dev), torch.from_numpy(seeds.view(np.int32)).to(dev)
                res = quench.relink_device(N, t, tg, sd, min_dist=md, local_search=search, walk=n, out=t)
                torch.cuda.current_stream(dev).synchronize()
                assert res["state"] is t and "energy_hist" not in res
                ru.assert_equal(quench.to_numpy(res), want, what + ", in place", fields=ru.FIELDS)
                np.testing.assert_array_equal(tg.cpu().numpy(), g)  # the guides are the caller's
                q = abi.Relink()
                t2, o2 = torch.from_numpy(s).to(dev), torch.zeros((n, N * N), dtype=torch.uint8, device=dev)
                q.N, q.mode, q.n_chains, q.min_dist, q.local_search, q.walk = N, abi.MODE_BOARD, n, md, abi.HOP_LOCAL_SEARCH[search], n
                q.seeds, q.state_in, q.guide_in, q.state_out = sd.data_ptr(), t2.data_ptr(), tg.data_ptr(), o2.data_ptr()
                mcq_amd._lib.relink_device(q, torch.cuda.current_stream(dev))
                torch.cuda.current_stream(dev).synchronize()
                np.testing.assert_array_equal(o2.cpu().numpy(), want["state"])
                np.testing.assert_array_equal(t2.cpu().numpy(), s)  # out of place: the input is untouched


def test_the_largest_fall_and_rise_of_a_step():
    """At N = 32 the centre column (15, 15) has 31 + 31 + 31 + 30 = 123 aligned columns, the most a column of a board in range has and
    one less than the 4 (N - 1) = 124 the key is sized for.  On a board with every queen at height 0 and the centre queen at height 20
    (which no aligned column attacks: its distances end at 16) the step that brings the centre queen down rises by 123, and the step
    the other way falls by 123: the ends the packed key (delta + 128 above 10 bits of rho) must hold.  A second column (0, 1), not
    aligned with the centre, competes in both walks."""
    N, LARGEST = 32, 123
    centre = 15 * N + 15
    flat = np.zeros((1, N * N), dtype=np.uint8)
    up, guide_up = flat.copy(), flat.copy()
    up[0, centre] = 20
    guide_up[0, 1] = 5
    down, guide_down = flat.copy(), up.copy()
    guide_down[0, 1] = 5
    seeds = abi.seeds_for(3, 1)
    for name, s, g, sign in (("rise", up, guide_up, 1), ("fall", down, guide_down, -1)):
        want = ru.relink_many(N, s, g, seeds, min_dist=0, local_search="single")
        deltas = [st["delta"] for st in want["trace"][0]]
        assert len(deltas) == 2 and sign * LARGEST in deltas and deltas == sorted(deltas), (name, deltas)
        got = quench.relink_states(N, s, g, seeds, min_dist=0, local_search="single", hist=True)
        ru.assert_equal(got, want, f"the largest {name}")
        ru.assert_equal(got, quench.relink_host(N, s, g, seeds, min_dist=0, local_search="single", hist=True), f"the largest {name}: host code")
        assert LARGEST in np.abs(np.diff(got["energy_hist"][0, :3].astype(np.int64)))


def test_a_stream_of_its_own():
    import torch

    dev = torch.device("cuda", torch.cuda.current_device())
    N, n = 12, 70
    s, g, seeds, md, want = _neighbours(N, n, "pairs")
    t, tg, sd = torch.from_numpy(s).to(dev), torch.from_numpy(g).to(dev), torch.from_numpy(seeds.view(np.int32)).to(dev)
    torch.cuda.current_stream(dev).synchronize()
    st = torch.cuda.Stream(device=dev)
    res = quench.relink_device(N, t, tg, sd, min_dist=md, walk=n, hist=True, stream=st)
    st.synchronize()
    ru.assert_equal(quench.to_numpy(res), want, "a stream of its own")
    with pytest.raises(ValueError, match="distinct from guide_in"):
        quench.relink_device(N, t, tg, sd, out=tg)
    with pytest.raises(ValueError, match="guides"):
        quench.relink_device(N, t, tg[:5], sd)
    with pytest.raises(ValueError, match="seeds"):
        quench.relink_device(N, t, tg, sd[:5])
    with pytest.raises(ValueError, match="contiguous uint8 tensor on the GPU"):
        quench.relink_device(N, s, tg, sd)


@pytest.mark.parametrize("align", (True, False))
def test_the_pool_equals_its_host_form(align):
    import torch

    dev = torch.device("cuda", torch.cuda.current_device())
    N, n, rounds = 6, 64, 3
    s = ru.minima(N, n, 17)
    s[s == N - 1] = 200  # clamped
    seeds = abi.seeds_for(23, n)
    want = quench.relink_pool_host(N, s, seeds, rounds, align=align, partner_seed=5)
    assert want["n_replaced"].sum() > 0 and (want["n_replaced"] < n).all()  # some slots take the result and some keep theirs
    t, sd = torch.from_numpy(s).to(dev), torch.from_numpy(seeds.view(np.int32)).to(dev)
    got = quench.relink_pool(N, t, sd, rounds, align=align, partner_seed=5)
    np.testing.assert_array_equal(got["state"].cpu().numpy(), want["state"])
    np.testing.assert_array_equal(got["energy"].cpu().numpy(), want["energy"])
    assert got["energy"].dtype == torch.int32 and got["state"].dtype == torch.uint8
    for k in ("n_replaced", "best_energy"):
        np.testing.assert_array_equal(got[k], want[k])
        assert got[k].dtype == want[k].dtype
    np.testing.assert_array_equal(t.cpu().numpy(), s)  # the caller's pool is untouched
    if align:  # the images on the device are those of the host
        ti, idx, dist = quench.nearest_image(N, t.clamp(max=N - 1), torch.roll(t.clamp(max=N - 1), 7, 0))
        hi, hidx, hdist = quench.nearest_image(N, np.minimum(s, N - 1), np.roll(np.minimum(s, N - 1), 7, axis=0))
        np.testing.assert_array_equal(ti.cpu().numpy(), hi)
        np.testing.assert_array_equal(idx.cpu().numpy(), hidx)
        np.testing.assert_array_equal(dist.cpu().numpy(), hdist)
        assert len(set(hidx.tolist())) > 4 and (hdist < (np.minimum(s, N - 1) != np.roll(np.minimum(s, N - 1), 7, axis=0)).sum(axis=1)).any()


def test_heat_bath_placements_through_the_invariants():
    """4 096 best_state boards of a heat-bath run at N = 12, each relinked with its neighbour, checked by kernels that share no code
    with the walk: consequences (c) and (d) of the rule."""
    import torch

    dev = torch.device("cuda", torch.cuda.current_device())
    N, n = 12, 4096
    seeds = abi.seeds_for(42, n)
    res = mcq_amd.heatbath.anneal_heatbath(N, 60, "random", {"type": "linear_annealing", "beta_start": 1.0, "beta_end": 3.0}, seeds)
    t = torch.from_numpy(np.ascontiguousarray(res["best_state"]).reshape(n, N * N)).to(dev)
    tg = torch.roll(t, -1, 0).contiguous()
    sd = torch.from_numpy(seeds.view(np.int32)).to(dev)
    w = quench.relink_device(N, t, tg, sd, min_dist=N * N // 8, hist=True)
    on_in, on_guide, on_best = (quench.quench_device(N, x, conflicts=False) for x in (t, tg, w["path_best_state"]))
    on_out = quench.quench_pairs_device(N, w["state"], conflicts=False)
    torch.cuda.current_stream(dev).synchronize()
    got, on_in, on_guide, on_best, on_out = (quench.to_numpy(x) for x in (w, on_in, on_guide, on_best, on_out))
    rows = np.arange(n)
    np.testing.assert_array_equal(got["energy_in"], on_in["energy_in"])
    np.testing.assert_array_equal(got["energy_in"], res["best_energy"])
    d0 = (res["best_state"].reshape(n, -1) != np.roll(res["best_state"].reshape(n, -1), -1, axis=0)).sum(axis=1)
    np.testing.assert_array_equal(got["distance_in"], d0)
    assert (got["n_steps"] == d0).all() and d0.min() > 2 * (N * N // 8)  # every walk has candidates
    # (b) the walk ends on the guide
    np.testing.assert_array_equal(got["energy_hist"][rows, d0], on_guide["energy_in"])
    # (d) path_best_energy is E of path_best_state, the smallest of the window, and L does not rise
    np.testing.assert_array_equal(got["path_best_energy"], on_best["energy_in"])
    np.testing.assert_array_equal(got["energy_hist"][rows, got["path_best_step"]], got["path_best_energy"])
    md = N * N // 8
    assert (got["path_best_step"] >= md).all() and (d0 - got["path_best_step"] >= md).all()
    hist = got["energy_hist"].astype(np.int64)
    window = np.where((np.arange(hist.shape[1])[None, :] >= md) & (np.arange(hist.shape[1])[None, :] <= (d0 - md)[:, None]), hist, 1 << 30)
    np.testing.assert_array_equal(window.min(axis=1), got["path_best_energy"])
    np.testing.assert_array_equal(window.argmin(axis=1), got["path_best_step"])  # the earliest of the smallest
    np.testing.assert_array_equal(hist.max(axis=1), got["path_max_energy"])
    assert (got["energy_out"] <= got["path_best_energy"]).all()
    # (c) state_out is a fixed point of L: the pair-move quench moves nothing on it and recounts its energy
    assert on_out["n_moves"].sum() == 0 and on_out["n_pair_moves"].sum() == 0 and (on_out["certified"] == 1).all()
    np.testing.assert_array_equal(on_out["energy_in"], got["energy_out"])
    print("below both endpoints:", int(((got["energy_out"] < got["energy_in"]) & (got["energy_out"] < on_guide["energy_in"])).sum()), "of", n,
          "barrier mean:", float((got["path_max_energy"] - got["energy_in"]).mean()))
