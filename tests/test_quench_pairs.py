"""GPU: the pair-move quench kernel (mcq_quench_pairs_device) against the library's host code (mcq_quench_pairs_host) bit for bit on every
output at both ends of every instantiation, in place and on a stream of its own; through invariants alone on the best placements of a
heat-bath run; and behind the annealing hooks (quench="pairs") against the composed calls.

Held independently of the library: at N = 17, 24, 25, 32 the kernel runs to certified = 1 and equals the NumPy restatement with the
exhaustive scan (tests/quench_pairs_util.py) on inputs whose coverage is asserted first, and its outputs pass the restatement's own
certificate; up to N = 6 it equals the restatement with the scan over all pairs.  At N = 7 .. 16 the kernel meets the restatement only
through the host code, which tests/test_quench_pairs_host.py compares with it at N = 8, 9, 12, 13, 16."""
import os

import numpy as np
import pytest

import mcq_amd
from tests import quench_pairs_util as qp
from tests import quench_util as qu
from tests import resume_util as ru

abi = mcq_amd.abi
quench = mcq_amd.quench
pytestmark = pytest.mark.gpu
LIN = {"type": "linear_annealing", "beta_start": 1.0, "beta_end": 3.0}

# the instantiations are padded N = 4, 8, 12, 16, 24, 32: both ends of each
SIZES = (2, 3, 4, 5, 8, 9, 12, 13, 16, 17, 24, 25, 32)


def _boards(N, n, seed):
    s = qu.random_boards(N, n, seed, over=True)  # bytes >= N among them
    s[0] = seed % N  # all heights equal
    if n > 2:
        s[1] = 255  # every byte clamped
    return s


@pytest.mark.parametrize("N", SIZES)
def test_kernel_equals_the_host_code(N):
    import torch

    max_rounds = 0 if N <= 16 else 2  # to convergence where the host scan is quick
    dev = torch.device("cuda", torch.cuda.current_device())
    for idx, n in enumerate((1, 5, 65)):
        s = _boards(N, n, 100 * N + idx)
        want = quench.quench_pairs_host(N, s, max_rounds=max_rounds)
        got = quench.quench_pairs(N, s, max_rounds=max_rounds)
        what = f"N={N}, {n} chains, max_rounds={max_rounds}"
        qp.assert_equal(got, want, what)
        for k in qp.FIELDS:
            assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        if max_rounds == 0:
            assert (got["certified"] == 1).all()
            one = quench.quench_pairs(N, s, max_rounds=1)
            qp.assert_equal(one, quench.quench_pairs_host(N, s, max_rounds=1), what + ", then max_rounds=1")
            assert (one["n_rounds"] == 1).all()
        # in place, and only the placements: every per-chain output is optional
        t = torch.from_numpy(s).to(dev)
        res = quench.quench_pairs_device(N, t, max_rounds=max_rounds, out=t)
        torch.cuda.current_stream(dev).synchronize()
        assert res["state"] is t
        qp.assert_equal(quench.to_numpy(res), want, what + ", in place")
        q = abi.QuenchPairs()
        t2, o2 = torch.from_numpy(s).to(dev), torch.zeros((n, N * N), dtype=torch.uint8, device=dev)
        q.N, q.mode, q.n_chains, q.max_rounds, q.state_in, q.state_out = N, abi.MODE_BOARD, n, max_rounds, t2.data_ptr(), o2.data_ptr()
        mcq_amd._lib.quench_pairs_device(q, torch.cuda.current_stream(dev))
        torch.cuda.current_stream(dev).synchronize()
        np.testing.assert_array_equal(o2.cpu().numpy(), want["state"])
        np.testing.assert_array_equal(t2.cpu().numpy(), s)  # out of place: the input is untouched
    if N <= 6:  # against the restatement too, where it is quick
        s = _boards(N, 3, 7 * N)
        qp.assert_equal(quench.quench_pairs(N, s), qp.quench_pairs_many(N, s), f"N={N} vs the restatement")


@pytest.mark.parametrize("N", (17, 24, 25, 32))
def test_kernel_converges_beyond_16_certified_without_the_library(N):
    """mcq_quench_pairs_kernel<24> and <32> to certified = 1 (max_rounds = 0) on minima with a few columns redrawn: against the host code
    and against the restatement with the exhaustive scan, on 1, 3 and 67 chains; the outputs certified by that scan and the single-move
    table, which owe nothing to the library.  Before any of it counts, the restatement's traces of the group must hold every class of
    pair move, every line of the board, the last dword of a table row, neighbouring columns and the second trip of the lane loop."""
    NP = qp.padded(N)
    cov = qp.Coverage()
    for M in qp.GROUPS[NP]:
        cov.add(M, qp.restated_case(M)[1])
    print(NP, cov.check(NP, qp.GROUPS[NP][1]))
    s, want = qp.restated_case(N)
    host = quench.quench_pairs_host(N, s)
    qp.assert_equal(host, want, f"N={N}: host code vs the restatement")
    assert int(host["n_rounds"].max()) >= 3
    for n in (1, 3, 67):
        rows = np.arange(n) % s.shape[0]
        got = quench.quench_pairs(N, s[rows])
        qp.assert_equal(got, {k: host[k][rows] for k in qp.FIELDS}, f"N={N}, {n} chains, to convergence")
        qp.assert_equal(got, {k: want[k][rows] for k in qp.FIELDS}, f"N={N}, {n} chains, vs the restatement")
        assert (got["certified"] == 1).all() and (got["n_rounds"] == got["n_pair_moves"] + 1).all()
    for r in (0, 1, 2, 66):  # chain 66 repeats board 0 behind the first 64 workgroups
        qp.certify(N, got["state"][r], f"N={N} chain {r}: a certified output of the kernel")
        assert qu.energy(N, got["state"][r]) == int(got["energy_out"][r])


def test_pair_moves_fire_on_the_device():
    """What the kernel is compared on is not vacuous: random boards make pair moves, several rounds of them."""
    for N, n, seed in ((4, 40, 2), (6, 16, 4), (12, 65, 5)):
        got = quench.quench_pairs(N, qu.random_boards(N, n, seed))
        assert 4 * int((got["n_pair_moves"] > 0).sum()) >= n and int(got["n_rounds"].max()) >= 3, N
        assert (got["energy_out"] + got["n_pair_moves"] <= got["energy_single"]).all()


def test_torch_tensors_on_a_side_stream(monkeypatch):
    """quench_pairs_device on a stream that is not the current one, with no synchronise inside."""
    import torch

    dev = torch.device("cuda", torch.cuda.current_device())
    s = qu.random_boards(12, 1031, 77, over=True)
    want = quench.quench_pairs_host(12, s)
    side = torch.cuda.Stream(dev)
    t = torch.from_numpy(s).to(dev)
    torch.cuda.synchronize()
    syncs = []
    real, real_all = torch.cuda.Stream.synchronize, torch.cuda.synchronize
    monkeypatch.setattr(torch.cuda.Stream, "synchronize", lambda self: (syncs.append("stream"), real(self))[1])
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: (syncs.append("device"), real_all(*a, **k))[1])
    res = quench.quench_pairs_device(12, t, stream=side)
    with torch.cuda.stream(side):
        res2 = quench.quench_pairs_device(12, res["state"], max_rounds=1, conflicts=False)  # (stream=None: torch's current stream, `side`)
    assert syncs == [], "quench_pairs_device synchronised"
    monkeypatch.undo()
    side.synchronize()
    qp.assert_equal(quench.to_numpy(res), want, "side stream")
    got2 = quench.to_numpy(res2)
    assert "conflicts" not in got2
    np.testing.assert_array_equal(got2["state"], want["state"])  # the output is a fixed point
    assert (got2["n_rounds"] == 1).all() and (got2["certified"] == 1).all() and (got2["n_moves"] == 0).all() and (got2["n_pair_moves"] == 0).all()


@pytest.fixture(scope="module")
def heatbath_run():
    """4 096 chains of N = 12 through a short heat-bath run, with the hook; shared by the tests below and left unchanged."""
    seeds = abi.seeds_for(42, 4096)
    plain = mcq_amd.heatbath.anneal_heatbath(12, 24, "random", LIN, seeds)
    hooked = mcq_amd.heatbath.anneal_heatbath(12, 24, "random", LIN, seeds, quench="pairs")
    return plain, hooked


def test_invariants_on_the_best_placements_of_a_heatbath_run(heatbath_run):
    import torch

    plain, _ = heatbath_run
    N, s = 12, plain["best_state"]
    dev = torch.device("cuda", torch.cuda.current_device())
    res = quench.quench_pairs_device(N, torch.from_numpy(s).to(dev))
    single = quench.quench_device(N, torch.from_numpy(s).to(dev), conflicts=False)
    again = quench.quench_device(N, res["state"])  # the single-move quench on the output
    torch.cuda.current_stream(dev).synchronize()
    got, single, again = quench.to_numpy(res), quench.to_numpy(single), quench.to_numpy(again)
    assert (again["n_moves"] == 0).all() and (again["n_passes"] == 1).all(), "the single-move quench moves an output"
    np.testing.assert_array_equal(again["state"], got["state"])
    np.testing.assert_array_equal(again["energy_in"], got["energy_out"])  # the recount of the output, by another kernel
    np.testing.assert_array_equal(again["conflicts"], got["conflicts"])
    np.testing.assert_array_equal(got["energy_in"], plain["best_energy"])
    np.testing.assert_array_equal(got["energy_single"], single["energy_out"])
    assert (got["energy_out"] <= got["energy_single"]).all() and (got["certified"] == 1).all()
    assert (got["n_rounds"] == got["n_pair_moves"] + 1).all()
    assert (got["energy_single"] - got["energy_out"] >= got["n_pair_moves"]).all()
    assert ((got["n_pair_moves"] == 0) == (got["energy_out"] == got["energy_single"])).all()
    where = got["n_pair_moves"] == 0  # nothing beyond the first descent: the output is the single-move quench's
    np.testing.assert_array_equal(got["state"][where], single["state"][where])
    for r in (0, 2047, 4095):
        assert ru.recount("board", N, got["state"][r]) == int(got["energy_out"][r])
    print(f"N=12, 4096 best_state boards behind 24 heat-bath sweeps: median energy {int(np.median(got['energy_single']))} -> "
          f"{int(np.median(got['energy_out']))}, improved {float((got['energy_out'] < got['energy_single']).mean()):.3f}, "
          f"most rounds {int(got['n_rounds'].max())}")


HOOK_FIELDS = {"quenched_state": "state", "quenched_energy": "energy_out", "quench_moves": "n_moves", "quench_pair_moves": "n_pair_moves",
               "quench_rounds": "n_rounds", "quench_certified": "certified", "quench_energy_single": "energy_single"}


def _assert_hook(res, plain, N, what):
    assert set(res) == set(plain) | set(HOOK_FIELDS) and not (set(HOOK_FIELDS) & set(plain)), what
    for k, v in plain.items():
        np.testing.assert_array_equal(res[k], v, err_msg=f"{what}: {k} changed with quench='pairs'")
    want = quench.quench_pairs(N, res["best_state"])
    for k, f in HOOK_FIELDS.items():
        np.testing.assert_array_equal(res[k], want[f], err_msg=f"{what}: {k}")
    np.testing.assert_array_equal(want["energy_in"], res["best_energy"])


def test_hooks_equal_the_composed_calls(heatbath_run, tmp_path):
    plain, hooked = heatbath_run
    _assert_hook(hooked, plain, 12, "anneal_heatbath")
    single = mcq_amd.heatbath.anneal_heatbath(12, 24, "random", LIN, abi.seeds_for(42, 4096)[:64], quench=True)
    assert set(single) == set(plain) | {"quenched_state", "quenched_energy", "quench_moves"}  # quench=True is what it was
    np.testing.assert_array_equal(single["quenched_energy"], quench.quench_pairs(12, single["best_state"])["energy_single"])
    # with resampling
    seeds = abi.seeds_for(7, 64)
    kw = dict(resample_every=6, population=32, resample_seed=3)
    p2, lin0 = mcq_amd.heatbath.anneal_heatbath(9, 18, "random", LIN, seeds, **kw)
    r2, lin1 = mcq_amd.heatbath.anneal_heatbath(9, 18, "random", LIN, seeds, quench="pairs", **kw)
    _assert_hook(r2, p2, 9, "anneal_heatbath with resampling")
    for k, v in lin0.items():
        np.testing.assert_array_equal(np.asarray(lin1[k]), np.asarray(v), err_msg=f"lineage {k}")
    # tempered
    ladder = [0.5, 1.0, 1.5, 2.0]
    p3 = mcq_amd.tempering.anneal_tempered(12, 20, "random", LIN, seeds, ladder, exchange_every=2)
    r3 = mcq_amd.tempering.anneal_tempered(12, 20, "random", LIN, seeds, ladder, exchange_every=2, quench="pairs")
    _assert_hook(r3, p3, 12, "anneal_tempered")
    # population annealing and the competition driver
    pk = dict(population=32, resample_seed=1, mcmc_type="board")
    p4, _ = mcq_amd.population.anneal_population(8, 2000, "random", LIN, seeds, 500, **pk)
    r4, _ = mcq_amd.population.anneal_population(8, 2000, "random", LIN, seeds, 500, quench="pairs", **pk)
    _assert_hook(r4, p4, 8, "anneal_population")
    energy, heights, path, info = mcq_amd.drivers.run_competition(N=8, n_runs=64, n_steps=2000, base_seed=7, out_dir=str(tmp_path), timestamp="t",
                                                                  resample_every=500, population=32, resample_seed=1, quench="pairs")
    r = int(np.argmin(r4["quenched_energy"]))
    assert os.path.basename(path) == "best_heights_8_t_quenched_pairs.txt" and os.path.exists(path)
    assert ru.recount("board", 8, heights.ravel()) == energy == int(r4["quenched_energy"].min())
    assert info == {"quenched": "pairs", "run": r, "energy_before": int(r4["best_energy"][r]), "moves": int(r4["quench_moves"][r]),
                    "pair_moves": int(r4["quench_pair_moves"][r]), "certified": True}
    np.testing.assert_array_equal(heights.ravel(), r4["quenched_state"][r])
    # ... and over independent chains, where the driver itself calls the quench
    e2, h2, path2, info2 = mcq_amd.drivers.run_competition(N=8, n_runs=32, n_steps=1500, out_dir=str(tmp_path), timestamp="u", quench="pairs")
    e1, _, _, info1 = mcq_amd.drivers.run_competition(N=8, n_runs=32, n_steps=1500, out_dir=str(tmp_path), timestamp="v", quench=True)
    assert ru.recount("board", 8, h2.ravel()) == e2 <= e1 and info2["quenched"] == "pairs" and info2["certified"] and info1["quenched"] is True
    assert "quenched_pairs" in os.path.basename(path2)
