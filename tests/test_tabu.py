"""GPU: the tabu kernel (mcq_tabu_device) against the library's host code (mcq_tabu_host) bit for bit on every output, histories and
tabu_out included, at both ends of every instantiation, and chain 0 of every such case against the restatement of tests/tabu_util.py
over the whole run; sleeping runs that wake at iteration 2^15 of one call, at both ends of the instantiations 12 to 32, whole, cut one
iteration before the base moves and at it, ending at it, and through 2^16 iterations up to N = 13; long runs in which the stamp base
moves twice with moves throughout (N = 4, 5, 9, 13); the top of the 16-bit stamp range and tabu_in at the contract's ends; the largest
fall and the largest rise the packed key can hold; first_iter on both sides of 2^32; a cut run at N = 12; in place; a stream of its
own; 4 096 heat-bath placements through the invariants of the rule; and the run_competition hook against the composed calls.  Before a
comparison counts its coverage is asserted, from the restatement's traces (tests/tabu_cases.py) or, where stated, from the host code's
counters and histories; none is computed from the kernel's outputs."""
import functools
import os

import numpy as np
import pytest

import mcq_amd
from tests import quench_util as qu
from tests import resume_util as ru
from tests import tabu_cases as tc
from tests import tabu_util as tu

abi = mcq_amd.abi
quench = mcq_amd.quench
pytestmark = pytest.mark.gpu

GROUPS = tc.GROUPS
ALL = tc.ALL
_iters, _stamps = tc.iters, tc.stamps


@functools.lru_cache(maxsize=None)
def _reference(N):
    """[(boards, seeds, keywords, the host code's result, the restatement's whole run of chain 0)] at N; computed once and shared."""
    out = []
    for i, (s, seeds, kw) in enumerate(tc.cases(N)):
        want = quench.tabu_host(N, s, seeds, _iters(N), **ALL, **kw)
        traced = tc.restated(N, i, 0)
        assert len(traced["trace"]) == _iters(N)
        tu.assert_equal(tc.row(want, 0), traced, f"N={N} case {i}: host code against the restatement")
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
        for s, seeds, kw, want, traced in _reference(N):
            assert int(s.max()) >= N or s.shape[0] < 65  # clamped bytes among the random inputs
            got = quench.tabu_states(N, s, seeds, _iters(N), **ALL, **kw)
            what = f"N={N} chains={s.shape[0]}"
            tu.assert_equal(got, want, what)
            tu.assert_equal(tc.row(got, 0), traced, what + ": chain 0 against the restatement")
            assert set(got) == set(quench.FIELDS_TABU)
            for k, dt in abi.TABU_DTYPES.items():
                assert got[k].dtype == dt, k
            slim = quench.tabu_states(N, s, seeds, _iters(N), **kw)
            assert "energy_hist" not in slim and "tabu_out" not in slim
            tu.assert_equal(slim, want, what + " without the optional outputs", fields=[k for k in tu.FIELDS if k in slim])


@pytest.mark.parametrize("N", (4, 5, 9, 13))
def test_the_stamp_base_moves_twice(N):
    """70 000 iterations under the longest tenure: the base of the kernel's 16-bit stamps moves at iterations 32 768 and 65 536, and
    stamps of 32 767 + 1 + 8192 + 4095 are written before a move.  Then the same run cut at 32 767 + 2 + rest, tabu_out carried: the
    second piece starts one iteration before the whole run's base moves, with the stamps the first piece left.  At N = 9 and 13 (the
    instantiations 12 and 16) with tenure_conf = 64 on top."""
    n, iters = 5, 70000
    s, seeds = qu.random_boards(N, n, 30 + N, over=True), abi.seeds_for(40 + N, n)
    kw = dict(tenure=8192, tenure_rand=4095) if N <= 5 else dict(tu.LONGEST)
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


@pytest.mark.parametrize("variant", tc.VARIANTS)
@pytest.mark.parametrize("N", sorted(tc.SLEEP_CHAINS))
def test_the_kernel_wakes_at_iteration_2_15(N, variant):
    """Sleeping runs (tests/tabu_util.py) at both ends of the instantiations 12, 16, 24 and 32: every stamp expires around iteration
    2^15 of ONE call, so the kernel moves its base with stamps of the longest tenure alive, written just before, and with stamps that
    expire exactly at, one before and one or two after the move.  The kernel equals the host code and the restated window on every
    output; so do the run cut one iteration before the move and at it, and a call that ends at the move."""
    print(N, variant, tc.check_wakes(N, variant))
    s, seeds, tin, W, want = tc.sleep_case(N, variant)
    kw = tc.sleep_kw(N, variant)
    host = quench.tabu_host(N, s, seeds, tc.SLEEP_ITERS, **ALL, **kw)
    tu.assert_asleep(host, W, f"N={N} {variant}")
    tu.assert_equal(host, want, f"N={N} {variant}: host code against the restated window")
    got = quench.tabu_states(N, s, seeds, tc.SLEEP_ITERS, **ALL, **kw)
    tu.assert_equal(got, host, f"N={N} {variant}: {tc.SLEEP_ITERS} iterations")
    tu.assert_equal(got, want, f"N={N} {variant}: against the restated window")
    for cuts in ((tu.REBASE - 1, 2, tc.SLEEP_ITERS - tu.REBASE - 1), (tu.REBASE, tc.SLEEP_ITERS - tu.REBASE)):
        parts = tu.run_cut(quench.tabu_states, N, s, seeds, cuts, **ALL, **kw)
        tu.assert_equal(tu.merge(parts), want, f"N={N} {variant}: cut {cuts}")
    ends = tc.sleep_case(N, variant, tu.REBASE)[4]  # the call that ends where the base would move: the restated window is [W, 2^15)
    assert int(ends["tabu_out"].max()) > 8192
    tu.assert_equal(quench.tabu_states(N, s, seeds, tu.REBASE, **ALL, **kw), ends, f"N={N} {variant}: {tu.REBASE} iterations")
    if N <= 13:  # the second move of the base, against the host code (tests/test_tabu_host.py: its cut at 2^15 is the whole)
        twice = quench.tabu_host(N, s, seeds, 2 * tu.REBASE, **ALL, **kw)
        assert (np.diff(twice["energy_hist"].astype(np.int64)[:, tc.SLEEP_ITERS:], axis=1) != 0).any(axis=1).all() and int(twice["tabu_out"].max()) > 0
        tu.assert_equal(quench.tabu_states(N, s, seeds, 2 * tu.REBASE, **ALL, **kw), twice, f"N={N} {variant}: {2 * tu.REBASE} iterations")


@pytest.mark.parametrize("N", (25, 32))
def test_the_top_of_the_stamp_range(N):
    """tabu_in with 65535, 65534, 32769, 32768, 32767, 1 and 0 among stamps that expire around iteration 2^15, nearly every column
    conflicting and the three tenure terms at their maxima: the moves just before the base moves write base-relative stamps within
    1024 of the largest there can be (at N = 32: of 2^15 + 2^14), and the base then moves under them and under the 65535s."""
    top, bound = tc.top_stamp(N)
    assert top >= bound and (N != 32 or bound == (1 << 15) + (1 << 14) - 1024), (top, bound)
    s, seeds, tin, W, want = tc.top_case(N)
    kw = dict(tabu_in=tin, best_floor=np.zeros(1, dtype=np.int32), **tu.LONGEST)
    host = quench.tabu_host(N, s, seeds, tc.TOP_ITERS, **ALL, **kw)
    tu.assert_asleep(host, W, f"N={N}")
    tu.assert_equal(host, want, f"N={N}: host code against the restated window")
    moved = np.flatnonzero(np.diff(host["energy_hist"][0].astype(np.int64)) != 0)
    assert ((moved >= W) & (moved < tu.REBASE)).sum() >= 60 and (moved >= tu.REBASE).sum() >= 300 and int(host["tabu_out"].max()) == 65535 - tc.TOP_ITERS
    got = quench.tabu_states(N, s, seeds, tc.TOP_ITERS, **ALL, **kw)
    tu.assert_equal(got, host, f"N={N}: the top of the stamp range")
    tu.assert_equal(got, want, f"N={N}: against the restated window")


def test_no_iterations_is_the_recount():
    """tabu_in over the whole uint16 range goes through a call of no iterations as it is."""
    for N, n in ((5, 4), (13, 2), (32, 1)):
        s = qu.random_boards(N, n, 9 + N, over=True)
        tin = np.random.RandomState(N).randint(0, 1 << 16, size=(n, N ** 3)).astype(np.uint16)
        tin[:, :4] = (65535, 32768, 32767, 0)
        seeds = abi.seeds_for(1, n)
        got = quench.tabu_states(N, s, seeds, 0, tenure=5, first_iter=(1 << 40) + 3, tabu_in=tin, **ALL)
        clamped = np.minimum(s, N - 1)
        np.testing.assert_array_equal(got["state"], clamped)
        np.testing.assert_array_equal(got["best_state"], clamped)
        np.testing.assert_array_equal(got["tabu_out"], tin)
        e = np.array([qu.energy(N, b) for b in s])
        for k in ("energy_in", "energy_out", "best_energy"):
            np.testing.assert_array_equal(got[k], e, err_msg=k)
        np.testing.assert_array_equal(got["energy_hist"], e[:, None])
        for k in tu.COUNTERS + ("best_iter",):
            assert not got[k].any(), k
        tu.assert_equal(got, quench.tabu_host(N, s, seeds, 0, tenure=5, first_iter=(1 << 40) + 3, tabu_in=tin, **ALL), f"N={N}: n_iters=0")
        floor = e - np.arange(n, dtype=np.int64) + 1  # above, at and below the recount
        np.testing.assert_array_equal(quench.tabu_states(N, s, seeds, 0, best_floor=floor.astype(np.int32))["best_energy"], np.minimum(floor, e))


@pytest.mark.parametrize("N", tc.KEY_N)
def test_the_largest_fall_and_the_largest_rise(N):
    """The ends of the key (delta + 124) << 15 | rho: delta = -max a(c, k) from the flat board and +(max a(c, k) - 3) back onto it,
    -123 and +120 at N = 32, with ties among such candidates."""
    for kind in ("flat", "uphill"):
        print(N, kind, tc.check_key(N, kind))
        b, seeds, kw, want = tc.key_case(N, kind)
        host = quench.tabu_host(N, b, seeds, tc.KEY_ITERS[kind], **ALL, **kw)
        tu.assert_equal(host, want, f"N={N} {kind}: host code against the restatement")
        got = quench.tabu_states(N, b, seeds, tc.KEY_ITERS[kind], **ALL, **kw)
        tu.assert_equal(got, want, f"N={N} {kind}")
        tu.assert_equal(got, host, f"N={N} {kind}: against the host code")


@pytest.mark.parametrize("N,n,first", tc.WORD_CASES)
def test_first_iter_on_both_sides_of_2_32(N, n, first):
    """The second word of the Philox counter is not 0: whole and cut 7 + 1 + 52 against the restatement and the host code, and not
    the run that a counter without its high word would give."""
    s, seeds, want = tc.word_case(N, n, first)
    low = tc.low_word_hist(tu.tabu_many, N, s, seeds, first)
    assert (want["energy_hist"] != low).any(axis=1).all(), "the high word decides nothing in these runs"
    kw = dict(first_iter=first, **tc.WORD_TENURE)
    host = quench.tabu_host(N, s, seeds, tc.WORD_ITERS, **ALL, **kw)
    tu.assert_equal(host, want, f"N={N} first_iter={first}: host code against the restatement")
    got = quench.tabu_states(N, s, seeds, tc.WORD_ITERS, **ALL, **kw)
    tu.assert_equal(got, want, f"N={N} first_iter={first}")
    tu.assert_equal(got, host, f"N={N} first_iter={first}: against the host code")
    parts = tu.run_cut(quench.tabu_states, N, s, seeds, (7, 1, 52), **ALL, **kw)
    tu.assert_equal(tu.merge(parts), want, f"N={N} first_iter={first}: cut")
    dropped = tc.low_word_hist(quench.tabu_states, N, s, seeds, first, **ALL)
    np.testing.assert_array_equal(dropped, low)
    assert (dropped != got["energy_hist"]).any(axis=1).all()


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
