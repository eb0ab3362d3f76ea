"""GPU: population annealing (mcq_resample_device through population.anneal_population) against the NumPy restatement of the rule, against
a run composed on the host from _lib.run_host_from segments, and -- where every plan is the identity -- against the CPU oracle's
unbroken chains; the four resampling kernels directly, at every kind of population size and table and in the one call the driver makes at a
boundary, between guard bytes.  Everything is bit for bit."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import mcq_amd
from tests import population_util as pu
from tests import resume_util as ru
from tests import util

abi = mcq_amd.abi
pop = mcq_amd.population
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIN = {"type": "linear_annealing", "beta_start": 1.0, "beta_end": 3.0}
EXP = {"type": "exponential_annealing", "beta_start": 0.5, "beta_end": 4.0}
SIN = {"type": "sinusoidal_annealing", "beta_start": 0.3, "beta_end": 4.0}


def _resample_on_device(energies, R, tab, offsets, state=None):
    """One mcq_resample_device call with torch tensors; returns (parent, stats, state_out, energy_out) as NumPy arrays."""
    import torch

    dev = torch.device("cuda", torch.cuda.current_device())
    st = torch.cuda.current_stream(dev)
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt).view(np.int32 if dt is np.uint32 else dt)).to(dev)  # noqa: E731
    n = len(energies)
    e, t, x = up(energies, np.int32), up(tab, np.uint32), up(offsets, np.uint32)
    sb = 16 if state is None else state.shape[1]
    s_in = up(np.zeros((n, sb), dtype=np.uint8) if state is None else state, np.uint8)
    s_out = torch.full((n, sb), 0xEE, dtype=torch.uint8, device=dev)
    parent = torch.full((n,), -1, dtype=torch.int32, device=dev)
    stats = torch.full((n // R, 3), -1, dtype=torch.int64, device=dev)
    e_out = torch.full((n,), -1, dtype=torch.int32, device=dev)
    r = abi.Resample()
    r.n_chains, r.population, r.state_bytes, r.table, r.table_len = n, R, sb, t.data_ptr(), len(tab)
    r.offsets, r.energies, r.state_in, r.state_out = x.data_ptr(), e.data_ptr(), s_in.data_ptr(), s_out.data_ptr()
    r.parent, r.stats, r.energy_out = parent.data_ptr(), stats.data_ptr(), e_out.data_ptr()
    scratch = torch.empty(int(mcq_amd._lib.lib().mcq_resample_scratch_bytes(ctypes.byref(r))), dtype=torch.uint8, device=dev)
    mcq_amd._lib.resample_device(r, scratch, st)
    st.synchronize()
    return parent.cpu().numpy(), stats.cpu().numpy(), s_out.cpu().numpy(), e_out.cpu().numpy()


def test_plan_kernel_equals_the_restatement():
    for name, e, R, tab, x in pu.plan_vectors():
        want_p, want_s = pu.plan(e, R, tab, x)
        got_p, got_s, _, e_out = _resample_on_device(e, R, tab, x)
        np.testing.assert_array_equal(got_p, want_p, err_msg=f"{name}: parents")
        np.testing.assert_array_equal(got_s, want_s, err_msg=f"{name}: distinct parents, W, E_min")
        np.testing.assert_array_equal(e_out, np.asarray(e)[want_p], err_msg=f"{name}: gathered energies")
        host_p, host_s = mcq_amd._lib.resample_plan_host(e, R, tab, x)
        np.testing.assert_array_equal(got_p, host_p, err_msg=f"{name}: kernel vs host code")
        np.testing.assert_array_equal(got_s, host_s, err_msg=f"{name}: kernel vs host code, stats")


RUN_FIELDS = ("best_energy", "steps_to_best", "n_accepted", "near_ties", "stream_words", "best_state")


def _guarded_call(energies, R, tab, offsets, state, first_step=0, seg=None, run=None, energy_out=True, fold=True, best_state=True):
    """One mcq_resample_device call as anneal_population issues it: plan, gather and (with seg / run) the fold in one call.  The scratch is
    exactly mcq_resample_scratch_bytes, and it and every array sit between 64-byte guard blocks, checked afterwards; every input, and
    every array the call was not given, must come back unchanged.  Returns the written arrays as NumPy arrays."""
    import torch

    dev = torch.device("cuda", torch.cuda.current_device())
    st = torch.cuda.current_stream(dev)
    n, sb = len(energies), state.shape[1]
    ins = {"energies": np.ascontiguousarray(energies, dtype=np.int32), "table": np.ascontiguousarray(tab, dtype=np.uint32),
           "offsets": np.ascontiguousarray(offsets, dtype=np.uint32), "state_in": np.ascontiguousarray(state, dtype=np.uint8)}
    outs = {"parent": np.full(n, -1, dtype=np.int32), "stats": np.full((n // R, 3), -1, dtype=np.int64),
            "state_out": np.full((n, sb), 0xEE, dtype=np.uint8), "energy_out": np.full(n, -1, dtype=np.int32)}
    for side, d in (("seg", seg), ("run", run)):
        for k in (d or {}):
            (ins if side == "seg" else outs)[f"{side}_{k}"] = d[k]
    r = abi.Resample()
    r.n_chains, r.population, r.state_bytes, r.table_len, r.first_step = n, R, sb, len(tab), int(first_step)
    absent = {k for k in outs if k.startswith("run_") and not fold} | {k for k in list(ins) + list(outs) if k.endswith("_best_state") and not best_state}
    absent |= set() if energy_out else {"energy_out"}
    bufs = {k: pu.guarded(torch, dev, a) for k, a in {**ins, **outs}.items()}
    for k, (_, view) in bufs.items():
        if k not in absent:
            setattr(r, k, view.data_ptr())
    exact = int(mcq_amd._lib.lib().mcq_resample_scratch_bytes(ctypes.byref(r)))
    assert exact == 8 * n
    bufs["scratch"] = pu.guarded(torch, dev, np.zeros(exact, dtype=np.uint8))
    assert bufs["scratch"][1].data_ptr() % 8 == 0 and all(bufs[k][1].data_ptr() % 16 == 0 for k in bufs)
    before = {k: buf.cpu().numpy().copy() for k, (buf, _) in bufs.items()}
    assert bufs["scratch"][1].numel() == exact
    mcq_amd._lib.resample_device(r, bufs["scratch"][1], st)
    st.synchronize()
    got = {}
    for k, (buf, _) in bufs.items():
        now = buf.cpu().numpy()
        assert (now[:64] == pu.GUARD).all() and (now[-64:] == pu.GUARD).all(), f"guard bytes around {k} were written"
        if k in ins or k in absent:
            np.testing.assert_array_equal(now, before[k], err_msg=f"{k} must not be written")
        if k in outs:
            got[k] = now[64:-64].view(outs[k].dtype).reshape(outs[k].shape).copy()
    return got


@pytest.mark.parametrize("group", pu.WIDE_GROUPS)
def test_plan_kernels_equal_the_restatement_on_the_wide_vectors(group):
    """The scan and the search kernel on tests/population_util.wide_vector_list(), whose conditions wide_plans() has asserted from the
    restatement: parents, all of stats and the gathered energies, against the restatement and against the host code.  The rows are each
    slot's own index, so state_out is the parents once more."""
    for v, want_p, want_s in pu.wide_plans():
        if v.group != group:
            continue
        n = len(v.energies)
        own = np.arange(n, dtype=np.int32)
        got = _guarded_call(v.energies, v.R, v.table, v.offsets, own.view(np.uint8).reshape(n, 4))
        np.testing.assert_array_equal(got["parent"], want_p, err_msg=f"{v.name}: parents")
        np.testing.assert_array_equal(got["stats"], want_s, err_msg=f"{v.name}: distinct parents, W, E_min")
        np.testing.assert_array_equal(got["energy_out"], v.energies[want_p], err_msg=f"{v.name}: gathered energies")
        np.testing.assert_array_equal(got["state_out"].view(np.int32).ravel(), want_p, err_msg=f"{v.name}: gathered rows")
        host_p, host_s = mcq_amd._lib.resample_plan_host(v.energies, v.R, v.table, v.offsets)
        np.testing.assert_array_equal(got["parent"], host_p, err_msg=f"{v.name}: kernel vs host code")
        np.testing.assert_array_equal(got["stats"], host_s, err_msg=f"{v.name}: kernel vs host code, stats")


def _boundary(first_step, state_bytes, **absent):
    """The boundary call on tests/population_util.boundary_vectors() and what the rule expects of it: (got, want, vectors)."""
    v = pu.boundary_vectors(first_step, state_bytes, seed=first_step % 1000 + state_bytes)
    c = v["counts"]
    assert len(v["energies"]) == 4160 and v["R"] == 1040 and c["equal"] >= 500 and c["lower"] >= 500 and c["moved"] >= 500, c
    got = _guarded_call(v["energies"], v["R"], v["table"], v["offsets"], v["state"], first_step, v["seg"], v["run"], **absent)
    p = v["parent"]
    want = {"parent": p, "stats": v["stats"], "state_out": v["state"][p], "energy_out": v["energies"][p]}
    want.update({f"run_{k}": a for k, a in pu.fold_rule(first_step, v["seg"], v["run"]).items()})
    return got, want, v


@pytest.mark.parametrize("first_step", (0, 5000))
@pytest.mark.parametrize("state_bytes", (36, 81, 144))
def test_boundary_call_as_the_driver_issues_it(first_step, state_bytes):
    """Plan, gather, the fold of best_state in the same rows kernel and the scalar fold in ONE call: 4 populations of 1 040 slots, rows of
    36, 81 and 144 bytes (4-, 1- and 16-byte lanes).  best_state is decided on the run's OLD best_energy although the scalar fold of the same
    call rewrites it: strictly lower moves the row, equal keeps it."""
    got, want, v = _boundary(first_step, state_bytes)
    assert sorted(got) == sorted(want) and all(("run_" + k) in want for k in RUN_FIELDS)
    if first_step:
        eq, lo = v["seg"]["best_energy"] == v["run"]["best_energy"], v["seg"]["best_energy"] < v["run"]["best_energy"]
        assert (want["run_best_state"][eq] == v["run"]["best_state"][eq]).all() and (want["run_best_state"][lo] == v["seg"]["best_state"][lo]).all()
        assert (want["run_best_energy"][lo] == v["seg"]["best_energy"][lo]).all()
    for k in want:
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"first_step {first_step}, rows of {state_bytes} bytes: {k}")


@pytest.mark.parametrize("absent", ("energy_out", "fold", "best_state"))
def test_boundary_call_leaves_absent_arrays_alone(absent):
    """The same call without energy_out, without the fold (run_* NULL: nothing of the run is written) and without seg / run_best_state
    while the scalars fold: the rest follows the rule, and what was not given is not written (_guarded_call checks it byte for byte)."""
    got, want, v = _boundary(5000, 81, **{absent: False})
    untouched = {"energy_out": ("energy_out",), "fold": tuple("run_" + k for k in RUN_FIELDS), "best_state": ("run_best_state",)}[absent]
    for k in want:
        if k not in untouched:
            np.testing.assert_array_equal(got[k], want[k], err_msg=f"without {absent}: {k}")
    for k in untouched:
        given = np.full(len(v["energies"]), -1, dtype=np.int32) if k == "energy_out" else v["run"][k[4:]]
        np.testing.assert_array_equal(got[k], given, err_msg=f"without {absent}: {k} was written")


def test_gather_kernel_moves_the_parents_rows():
    rs = np.random.RandomState(5)
    tab = abi.resample_table(0.05)
    p = abi.make_params(6, 1, "random", LIN, 16, mcmc_type="full_3d", Q=20)
    assert abi.state_bytes(p.N, p.mode, p.n_queens) == 60 and abi.state_bytes(5, abi.MODE_FULL3D) == 75
    # boards N = 6, 9, 12 (36, 81, 144 bytes: 4-, 1- and 16-byte lanes), full_3d N = 5 (75), full_3d Q != N^2 (N = 6, Q = 20 and 7: 60 and 21), N = 8 (192)
    for what, sb in (("board 6", 36), ("board 9", 81), ("board 12", 144), ("full_3d 5", 75), ("full_3d 6 Q=20", 60), ("full_3d 6 Q=7", 21), ("full_3d 8", 192)):
        for n, R in ((1024, 1024), (960, 48), (4096, 1024)):
            e = rs.randint(20, 120, size=n).astype(np.int32)
            state = rs.randint(0, 256, size=(n, sb)).astype(np.uint8)
            x = rs.randint(0, 2**32, size=n // R, dtype=np.uint32)
            parent, _, out, e_out = _resample_on_device(e, R, tab, x, state=state)
            want_p, _ = pu.plan(e, R, tab, x)
            np.testing.assert_array_equal(parent, want_p, err_msg=what)
            assert (parent != np.arange(n)).any(), f"{what}: the vector resamples nothing"
            np.testing.assert_array_equal(out, state[want_p], err_msg=f"{what}: state_out != state_in[parent] ({n} chains in populations of {R})")
            np.testing.assert_array_equal(e_out, e[want_p], err_msg=what)


CASES = (
    # N, mode, Q, schedule, chains, steps, S, population, trace, lanes
    (6, "board", None, LIN, 256, 2000, 300, None, True, 4),       # S does not divide n_steps
    (12, "board", None, EXP, 512, 3000, 500, 256, "reduced", 8),  # two populations
    (12, "board", None, SIN, 256, 2400, 400, None, False, 16),
    (12, "board", None, LIN, 1024, 3000, 250, 512, True, 0),
    (8, "full_3d", None, LIN, 256, 1500, 500, None, True, 8),
    (8, "full_3d", None, EXP, 256, 1300, 400, 128, "reduced", 16),
    (8, "full_3d", None, SIN, 256, 1200, 300, None, False, 4),
    (6, "full_3d", 20, LIN, 128, 1000, 250, 64, True, 0),
)


@pytest.mark.parametrize("N,mode,Q,sp,n,steps,S,R,trace,lanes", CASES)
def test_device_path_equals_the_host_composed_run(N, mode, Q, sp, n, steps, S, R, trace, lanes):
    seeds = abi.seeds_for(42, n)
    kw = dict(population=R, resample_seed=7, mcmc_type=mode, trace=trace, lanes_per_chain=lanes, Q=Q)
    got = pop.anneal_population(N, steps, "random", sp, seeds, S, **kw)
    want = pu.compose_host(N, steps, "random", sp, seeds, S, **kw)
    what = f"{mode} N={N} Q={Q} {sp['type']} {n}x{steps} S={S} R={R} trace={trace} G={lanes}"
    pu.assert_runs_equal(got, want, trace, what)
    res, lin = got
    assert int(res["near_ties"].sum()) == 0, f"{what}: near ties"
    assert (lin["parents"] != np.arange(n)[None, :]).any(), f"{what}: nothing was resampled"
    for r in (0, n // 2, n - 1):
        ru.assert_stream_is_numpys(res["stream_state"][r], int(seeds[r]), int(res["stream_words"][r]), f"{what}: chain {r}")


@pytest.mark.parametrize("mode,N", (("board", 12), ("full_3d", 8)))
def test_constant_schedule_is_the_oracles_unbroken_run(mode, N):
    """dbeta = 0 at every boundary: equal weights, every plan is the identity, and the run is the reference's own chains."""
    from oracle import oracle

    sp = {"type": "constant", "beta_const": 1.5}
    n, steps = 128, 2100
    seeds = abi.seeds_for(300, n)
    res, lin = pop.anneal_population(N, steps, "random", sp, seeds, 400, population=64, resample_seed=3, mcmc_type=mode, trace=True)
    want = oracle.run(abi.make_params(N, steps, "random", sp, n, mcmc_type=mode), seeds, n_threads=8)
    assert (lin["parents"] == np.arange(n)[None, :]).all() and (lin["distinct_parents"] == 64).all()
    assert (lin["weight_sum"] == 64 << 24).all() and (lin["ancestors"] == np.arange(n)).all()
    util.assert_results_equal(res, want, f"{mode} N={N}: constant schedule vs the oracle")  # history and accept bits included
    np.testing.assert_array_equal(res["stream_words"], want["stream_words"])
    assert int(res["near_ties"].sum()) == 0


def test_invariants_and_selection():
    """N = 12 board, 1 024 chains x 20 000 steps, linear 1 -> 3, S = 500: selection does something, and what a slot reports is what it held."""
    N, n, steps, S = 12, 1024, 20000, 500
    seeds = abi.seeds_for(42, n)
    res, lin = pop.anneal_population(N, steps, "random", LIN, seeds, S, mcmc_type="board", trace=True)
    par = lin["parents"]
    assert par.shape == (steps // S - 1, n)
    assert (par != np.arange(n)[None, :]).any(), "no boundary resampled anything"
    distinct = len(np.unique(lin["ancestors"]))
    print(f"distinct ancestors {distinct} of {n}; distinct parents per boundary {lin['distinct_parents'][:, 0].tolist()}; "
          f"best energy min {int(res['best_energy'].min())} median {int(np.median(res['best_energy']))}")
    assert distinct < n
    np.testing.assert_array_equal(lin["ancestors"], pop.ancestors_of(par, n))
    for k in range(1, len(lin["lengths"])):  # the segment starts from the parents' placements: the restore kernel's recount says so
        np.testing.assert_array_equal(lin["segment_initial_energy"][k], lin["segment_final_energy"][k - 1][par[k - 1]], err_msg=f"segment {k}")
        np.testing.assert_array_equal(lin["received_energy"][k - 1], lin["segment_initial_energy"][k])
        assert (np.diff(par[k - 1]) >= 0).all()
        assert int(lin["distinct_parents"][k - 1, 0]) == len(np.unique(par[k - 1])) and int(lin["e_min"][k - 1, 0]) == int(lin["segment_final_energy"][k - 1].min())
    for r in list(range(0, n, 97)) + [int(np.argmin(res["best_energy"]))]:
        assert ru.recount("board", N, res["final_state"][r]) == int(res["final_energy"][r]), r
        assert ru.recount("board", N, res["best_state"][r]) == int(res["best_energy"][r]), r
    # best_energy is the minimum of what the slot held: its stitched history and the energies it received at the boundaries (entry 0 of a
    # later segment, which the stitched history drops); steps_to_best is the first index of that minimum
    hist = res["energy_hist"][:, : steps + 1]
    np.testing.assert_array_equal(hist[:, -1], res["final_energy"])
    np.testing.assert_array_equal(hist[:, 0], res["initial_energy"])
    held = np.minimum(hist.min(axis=1), lin["received_energy"].min(axis=0))
    np.testing.assert_array_equal(res["best_energy"], held)
    best, stb, idx = res["best_energy"], res["steps_to_best"], np.arange(n)
    print(f"slots whose best energy is one they received and never saw again: {int((best < hist.min(axis=1)).sum())} of {n}")
    # in THIS run (seeded, hence the same everywhere) no slot is left with a received energy below everything its own history shows, so the
    # plain statement holds as well; in general a slot may move uphill from a parent's placement and never come back
    np.testing.assert_array_equal(best, hist.min(axis=1))
    at_own = hist[idx, stb] == best  # the best is an entry of the slot's own history: then the first one
    np.testing.assert_array_equal(stb[at_own], hist.argmin(axis=1)[at_own])
    k = stb[~at_own] // S  # ... or the energy received at boundary k, which the strict rule dates to step k S
    assert (stb[~at_own] % S == 0).all() and (k >= 1).all()
    np.testing.assert_array_equal(lin["received_energy"][k - 1, idx[~at_own]], best[~at_own])
    assert (res["best_energy"] <= hist.min(axis=1)).all()


def test_run_population_and_the_competition_writer(tmp_path):
    best, heights, path = mcq_amd.drivers.run_competition(N=12, n_runs=256, n_steps=6000, out_dir=str(tmp_path), timestamp="t", resample_every=500,
                                                          population=128, resample_seed=1)
    assert os.path.exists(path) and heights.shape == (12, 12)
    assert ru.recount("board", 12, heights.ravel()) == best
    res, _ = pop.anneal_population(12, 6000, "random", LIN, abi.seeds_for(42, 256), 500, population=128, resample_seed=1, mcmc_type="board")
    assert best == int(res["best_energy"].min())
    np.testing.assert_array_equal(heights.ravel(), res["best_state"][int(np.argmin(res["best_energy"]))])
    h, b, _, acc, rej, stb = mcq_amd.experiments.run_population(12, 6000, "random", None, 256, 500, population=128, resample_seed=1, base_seed=42,
                                                                 schedule_params=LIN, mcmc_type="board")
    assert b == [int(v) for v in res["best_energy"]] and stb == [int(v) for v in res["steps_to_best"]]
    assert all(len(h[r]) == 6001 and len(acc[r]) + len(rej[r]) == 6000 and len(acc[r]) == int(res["n_accepted"][r]) for r in range(256))


def test_anneal_population_in_a_fresh_process(tmp_path):
    out = str(tmp_path / "pop.npz")
    args = "12, 3000, 'random', %r, mcq_amd.abi.seeds_for(9, 256), 400" % (EXP,)
    code = ("import sys, numpy as np\nsys.path.insert(0, %r)\nimport mcq_amd\n"
            "res, lin = mcq_amd.population.anneal_population(%s, population=128, resample_seed=2, mcmc_type='board', trace='reduced')\n"
            "np.savez(%r, **res, **{'lin_' + k: v for k, v in lin.items() if isinstance(v, np.ndarray)})\n" % (ROOT, args, out))
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT, timeout=600)
    res, lin = pop.anneal_population(12, 3000, "random", EXP, abi.seeds_for(9, 256), 400, population=128, resample_seed=2, mcmc_type="board", trace="reduced")
    with np.load(out) as z:
        for k, v in res.items():
            np.testing.assert_array_equal(z[k], v, err_msg=k)
        for k in pu.LINEAGE_FIELDS:
            np.testing.assert_array_equal(z["lin_" + k], lin[k], err_msg=k)
