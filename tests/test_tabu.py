"""GPU: the tabu kernel (mcq_tabu_device) against the library's host code (mcq_tabu_host) bit for bit on every output, histories and
tabu_out included, at both ends of every instantiation; long runs in which the stamp base moves twice, whole and cut at the move; a cut
run at N = 12; in place; a stream of its own; 4 096 heat-bath placements through the invariants of the rule; and the run_competition
hook against the composed calls.  Before a group of comparisons counts it must hold aspired and uphill moves, a stall above E = 0 and a
new best behind a rise (from the host code's counters and histories), and winners that are not the row-major first of their ties and a
wrapped rho (from the restatement of tests/tabu_util.py on the first iterations of every first chain)."""
import functools
import os

import numpy as np
import pytest

import mcq_amd
from tests import quench_util as qu
from tests import resume_util as ru
from tests import tabu_util as tu

abi = mcq_amd.abi
quench = mcq_amd.quench
pytestmark = pytest.mark.gpu

# the instantiations are padded N = 4, 8, 12, 16, 24, 32: both ends of each
GROUPS = {4: (2, 4), 8: (5, 8), 12: (9, 12), 16: (13, 16), 24: (17, 24), 32: (25, 32)}
DEEP_FROM = 17     # from this N on the comparisons start deep in a walk: a short run from a random board only descends
DEEP_ITERS = 2500
DEEP_TENURE = dict(tenure=8, tenure_rand=4, tenure_conf=2)
TRACED = 40        # iterations of every first chain that the restatement follows
ALL = dict(hist=True, tabu_out=True)


def _iters(N):
    return 300 if N < DEEP_FROM else 200


def _stamps(N, n, seed, hold):
    """Random stamps of up to 40 iterations; chain 0 has every entry tabu for `hold` iterations."""
    tin = np.random.RandomState(seed).randint(0, 41, size=(n, N ** 3)).astype(np.uint16)
    tin[0] = hold
    return tin


@functools.lru_cache(maxsize=None)
def _deep(N):
    """3 boards of N >= DEEP_FROM behind DEEP_ITERS iterations of the host code, with their stamps and best energies: inputs only."""
    s = qu.random_boards(N, 3, 100 * N, over=True)
    return quench.tabu_host(N, s, abi.seeds_for(900 + N, 3), DEEP_ITERS, tabu_out=True, **DEEP_TENURE)


def _cases(N):
    """(boards, seeds, keywords) of the comparisons at N: every chain count; tenure = 8192 at N <= 3 and a start with every entry of a
    chain tabu under a floor of 0 are the stalls, random stamps the aspiration; at N >= DEEP_FROM the walk goes on from _deep."""
    if N >= DEEP_FROM:
        d = _deep(N)
        deep = dict(first_iter=DEEP_ITERS, tabu_in=d["tabu_out"], best_floor=d["best_energy"], **DEEP_TENURE)
        s = qu.random_boards(N, 3, 100 * N + 3, over=True)
        floor = np.full(3, 1 << 30, dtype=np.int32)
        floor[0] = 0
        return ((d["state"][:1], abi.seeds_for(900 + N, 1), {k: (v[:1] if isinstance(v, np.ndarray) else v) for k, v in deep.items()}),
                (d["state"], abi.seeds_for(900 + N, 3), deep),
                (s, abi.seeds_for(500 + N, 3), dict(tenure=3, tenure_rand=5, tabu_in=_stamps(N, 3, N, 50), best_floor=floor)))
    floor = np.full(5, 1 << 30, dtype=np.int32)
    floor[0] = 0
    return ((qu.random_boards(N, 1, 100 * N + 1, over=True), abi.seeds_for(500 + N, 1), dict(tenure=8192 if N <= 3 else N // 2 + 1, tenure_rand=3)),
            (qu.random_boards(N, 5, 100 * N + 5, over=True), abi.seeds_for(510 + N, 5), dict(tenure=2, tenure_rand=5, tenure_conf=8, tabu_in=_stamps(N, 5, N, 100),
                                                                                               best_floor=floor)),
            (qu.random_boards(N, 65, 100 * N + 65, over=True), abi.seeds_for(520 + N, 65), dict(tenure=N, tenure_rand=N, tenure_conf=4)))


@functools.lru_cache(maxsize=None)
def _reference(N):
    """[(boards, seeds, keywords, the host code's result, the restatement's first iterations of chain 0)] at N; computed once and shared."""
    out = []
    for s, seeds, kw in _cases(N):
        want = quench.tabu_host(N, s, seeds, _iters(N), **ALL, **kw)
        one = {k: (v[0] if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
        traced = tu.tabu(N, s[0], int(seeds[0]), TRACED, **one)
        np.testing.assert_array_equal(traced["energy_hist"], want["energy_hist"][0, : TRACED + 1])  # a run's beginning is a run
        out.append((s, seeds, kw, want, traced))
    return out


def _check_coverage(NP):
    cov, held = tu.Coverage(), dict.fromkeys(("aspired", "uphill", "stall_above_0", "best_after_uphill"), 0)
    for N in GROUPS[NP]:
        for _, _, _, want, traced in _reference(N):
            cov.add(NP, [traced["trace"]])
            for k, v in tu.counters_cover(want).items():
                held[k] += v
    n = dict(cov.n[NP], **held)
    for k, need in tu.Coverage.NEED.items():
        assert n[k] >= need, f"group {NP}: {k} = {n[k]} < {need}: {n}"
    return n


@pytest.mark.parametrize("NP", sorted(GROUPS))
def test_kernel_equals_the_host_code(NP):
    print(NP, _check_coverage(NP))
    for N in GROUPS[NP]:
        for s, seeds, kw, want, _ in _reference(N):
            assert int(s.max()) >= N or s.shape[0] < 65  # clamped bytes among the random inputs
            got = quench.tabu_states(N, s, seeds, _iters(N), **ALL, **kw)
            what = f"N={N} chains={s.shape[0]}"
            tu.assert_equal(got, want, what)
            assert set(got) == set(quench.FIELDS_TABU)
            for k, dt in abi.TABU_DTYPES.items():
                assert got[k].dtype == dt, k
            slim = quench.tabu_states(N, s, seeds, _iters(N), **kw)
            assert "energy_hist" not in slim and "tabu_out" not in slim
            tu.assert_equal(slim, want, what + " without the optional outputs", fields=[k for k in tu.FIELDS if k in slim])


@pytest.mark.parametrize("N", (4, 5))
def test_the_stamp_base_moves_twice(N):
    """70 000 iterations under the longest tenure: the base of the kernel's 16-bit stamps moves at iterations 32 768 and 65 536, and
    stamps of 32 767 + 1 + 8192 + 4095 are written before a move.  Then the same run cut at 32 767 + 2 + rest, tabu_out carried: the
    second piece starts one iteration before the whole run's base moves, with the stamps the first piece left."""
    n, iters = 5, 70000
    s, seeds = qu.random_boards(N, n, 30 + N, over=True), abi.seeds_for(40 + N, n)
    kw = dict(tenure=8192, tenure_rand=4095)
    want = quench.tabu_host(N, s, seeds, iters, **ALL, **kw)
    assert (want["n_stalled"] > 0).all() and (want["n_moves"] > 100).all() and want["n_uphill"].sum() > 0
    # moves on both sides of both marks, and stamps alive at the end
    moved = np.diff(want["energy_hist"].astype(np.int64), axis=1) != 0
    assert moved[:, :32768].any() and moved[:, 32768:65536].any() and moved[:, 65536:].any() and int(want["tabu_out"].max()) > 4096
    got = quench.tabu_states(N, s, seeds, iters, **ALL, **kw)
    tu.assert_equal(got, want, f"N={N}: {iters} iterations")
    parts = tu.run_cut(quench.tabu_states, N, s, seeds, (32767, 2, iters - 32769), **ALL, **kw)
    tu.assert_equal(tu.merge(parts), want, f"N={N}: 32 767 + 2 + rest")
    assert int(parts[0]["tabu_out"].max()) > 8192  # stamps that the second piece needs


def test_a_cut_run_is_the_unbroken_run():
    N, n = 12, 65
    s, seeds = qu.random_boards(N, n, 52, over=True), abi.seeds_for(9, n)
    kw = dict(tenure=6, tenure_rand=4, tenure_conf=4)
    tin = _stamps(N, n, 3, 20)
    whole = quench.tabu_host(N, s, seeds, 400, first_iter=4, tabu_in=tin, **ALL, **kw)
    parts = tu.run_cut(quench.tabu_states, N, s, seeds, (7, 1, 392), first_iter=4, tabu_in=tin, **ALL, **kw)
    tu.assert_equal(tu.merge(parts), whole, "N=12: 7 + 1 + 392 iterations")
    assert (whole["best_iter"] > 8).any() and whole["n_uphill"].sum() > 0


def test_in_place():
    import torch

    dev = torch.device("cuda", torch.cuda.current_device())
    N, n = 9, 67
    s, seeds = qu.random_boards(N, n, 5, over=True), abi.seeds_for(6, n)
    tin = _stamps(N, n, 8, 30)
    want = quench.tabu_host(N, s, seeds, 120, tenure=5, tenure_rand=2, tabu_in=tin, **ALL)
    t, sd = torch.from_numpy(s).to(dev), torch.from_numpy(seeds.view(np.int32)).to(dev)
    stamps = torch.from_numpy(tin.view(np.int16)).to(dev)
    res = quench.tabu_device(N, t, sd, 120, tenure=5, tenure_rand=2, tabu_in=stamps, out=t, **ALL)
    torch.cuda.current_stream(dev).synchronize()
    assert res["state"] is t
    tu.assert_equal(quench.tabu_to_numpy(res), want, "out = states")
    # the stamps in place too, and only the placements: every per-chain output is optional
    t = torch.from_numpy(s).to(dev)
    q = abi.Tabu()
    q.N, q.mode, q.n_chains, q.n_iters, q.tenure, q.tenure_rand = N, abi.MODE_BOARD, n, 120, 5, 2
    q.seeds, q.state_in, q.state_out, q.tabu_in, q.tabu_out = sd.data_ptr(), t.data_ptr(), t.data_ptr(), stamps.data_ptr(), stamps.data_ptr()
    mcq_amd._lib.tabu_device(q, torch.cuda.current_stream(dev))
    torch.cuda.current_stream(dev).synchronize()
    np.testing.assert_array_equal(t.cpu().numpy(), want["state"])
    np.testing.assert_array_equal(stamps.cpu().numpy().view(np.uint16), want["tabu_out"])


def test_torch_tensors_on_a_side_stream(monkeypatch):
    """tabu_device on a stream that is not the current one, with no synchronise inside."""
    import torch

    dev = torch.device("cuda", torch.cuda.current_device())
    N, n = 12, 257
    s, seeds = qu.random_boards(N, n, 77), abi.seeds_for(21, n)
    kw = dict(tenure=7, tenure_rand=3)
    want = quench.tabu_host(N, s, seeds, 150, **ALL, **kw)
    side = torch.cuda.Stream(dev)
    t, sd = torch.from_numpy(s).to(dev), torch.from_numpy(seeds.view(np.int32)).to(dev)
    torch.cuda.synchronize()
    syncs = []
    real, real_all = torch.cuda.Stream.synchronize, torch.cuda.synchronize
    monkeypatch.setattr(torch.cuda.Stream, "synchronize", lambda self: (syncs.append("stream"), real(self))[1])
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: (syncs.append("device"), real_all(*a, **k))[1])
    res = quench.tabu_device(N, t, sd, 150, stream=side, **ALL, **kw)
    with torch.cuda.stream(side):  # (stream=None: torch's current stream, `side`): the recount of what the call before left
        res2 = quench.tabu_device(N, res["state"], sd, 0, first_iter=150, tabu_in=res["tabu_out"], best_floor=res["best_energy"], **ALL, **kw)
    assert syncs == [], "tabu_device synchronised"
    monkeypatch.undo()
    side.synchronize()
    tu.assert_equal(quench.tabu_to_numpy(res), want, "side stream")
    got2 = quench.tabu_to_numpy(res2)
    for k in ("state", "tabu_out", "best_energy", "energy_out"):
        np.testing.assert_array_equal(got2[k], want[k], err_msg=k)
    np.testing.assert_array_equal(got2["energy_in"], want["energy_out"])
    with pytest.raises(ValueError, match="seeds"):
        quench.tabu_device(N, t, sd[:5], 1)
    with pytest.raises(ValueError, match="uint8 tensor"):
        quench.tabu_device(N, t.to(torch.int32), sd, 1)
    with pytest.raises(ValueError, match="tabu_in"):
        quench.tabu_device(N, t, sd, 1, tabu_in=res["tabu_out"][:5])
    with pytest.raises(ValueError, match="best_floor"):
        quench.tabu_device(N, t, sd, 1, best_floor=res["best_iter"])


def test_heat_bath_placements_through_the_invariants():
    """4 096 best_state boards of a heat-bath run at N = 12 x 500 iterations, checked by kernels that share no code with the walk."""
    import torch

    dev = torch.device("cuda", torch.cuda.current_device())
    N, n, iters = 12, 4096, 500
    seeds = abi.seeds_for(42, n)
    res = mcq_amd.heatbath.anneal_heatbath(N, 60, "random", {"type": "linear_annealing", "beta_start": 1.0, "beta_end": 3.0}, seeds)
    t = torch.from_numpy(np.ascontiguousarray(res["best_state"]).reshape(n, N * N)).to(dev)
    sd = torch.from_numpy(seeds.view(np.int32)).to(dev)
    w = quench.tabu_device(N, t, sd, iters, tenure=8, tenure_rand=4, hist=True)
    on_in, on_out, on_best = (quench.quench_device(N, x, conflicts=False) for x in (t, w["state"], w["best_state"]))
    torch.cuda.current_stream(dev).synchronize()
    got, on_in, on_out, on_best = quench.tabu_to_numpy(w), quench.to_numpy(on_in), quench.to_numpy(on_out), quench.to_numpy(on_best)
    hist = got["energy_hist"].astype(np.int64)
    np.testing.assert_array_equal(got["best_energy"], hist.min(axis=1))
    np.testing.assert_array_equal(got["best_iter"], hist.argmin(axis=1))
    assert (got["best_energy"] <= got["energy_in"]).all()
    np.testing.assert_array_equal(hist[:, 0], on_in["energy_in"])     # the history's ends are recounts of the quench kernel
    np.testing.assert_array_equal(hist[:, -1], on_out["energy_in"])
    np.testing.assert_array_equal(got["energy_out"], hist[:, -1])
    np.testing.assert_array_equal(got["best_energy"], on_best["energy_in"])
    np.testing.assert_array_equal(got["n_moves"] + got["n_stalled"], np.full(n, iters))
    np.testing.assert_array_equal(got["n_uphill"], (np.diff(hist, axis=1) > 0).sum(axis=1))
    applies = got["best_iter"] < iters
    assert applies.sum() > n // 2 and not on_best["n_moves"][applies].any(), "a single move lowers a best_state behind which an iteration ran"
    print("chains below their start:", int((got["best_energy"] < got["energy_in"]).sum()), "of", n, "min", int(got["best_energy"].min()), "from", int(got["energy_in"].min()))


def test_the_competition_hook_equals_the_composed_calls(tmp_path):
    kw = dict(N=8, n_runs=64, n_steps=2000, base_seed=7, out_dir=str(tmp_path))
    e0, h0, p0 = mcq_amd.drivers.run_competition(timestamp="a", **kw)
    assert os.path.basename(p0) == "best_heights_8_a.txt"  # tabu_iters=0: what it was
    e1, h1, p1, info = mcq_amd.drivers.run_competition(timestamp="b", tabu_iters=300, tabu_tenure=6, **kw)
    # the composed calls: the same search, then tabu_states on its best_state
    res, _ = mcq_amd.experiments.run_chains(8, 2000, "random", {"type": "linear_annealing", "beta_start": 1.0, "beta_end": 3.0}, abi.seeds_for(7, 64),
                                mcmc_type="board", early_stop_patience=None, trace=False, states=True)
    assert int(res["best_energy"].min()) == e0
    w = quench.tabu_states(8, res["best_state"], abi.seeds_for(7, 64), 300, tenure=6)
    r = int(np.argmin(w["best_energy"]))
    assert os.path.basename(p1) == "best_heights_8_b_tabu.txt" and os.path.exists(p1)
    assert e1 == int(w["best_energy"][r]) == ru.recount("board", 8, h1.ravel()) and e1 <= e0
    np.testing.assert_array_equal(h1.ravel(), w["best_state"][r])
    assert info == {"tabu": 300, "tenure": 6, "run": r, "energy_before": int(res["best_energy"][r]), "best_energy": e1, "best_iter": int(w["best_iter"][r]),
                    "moves": int(w["n_moves"][r]), "uphill": int(w["n_uphill"][r]), "aspired": int(w["n_aspired"][r]), "stalled": int(w["n_stalled"][r])}
    # behind the heat bath with the pair-move quench: both suffixes
    e2, h2, p2, info2 = mcq_amd.drivers.run_competition(timestamp="c", heatbath_sweeps=12, quench="pairs", tabu_iters=50, **kw)
    assert os.path.basename(p2) == "best_heights_8_c_quenched_pairs_tabu.txt" and info2["quenched"] == "pairs" and info2["tenure"] == 10
    assert ru.recount("board", 8, h2.ravel()) == e2 == info2["best_energy"] <= info2["energy_before"]
