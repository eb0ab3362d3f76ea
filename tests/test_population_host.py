"""CPU-only: population annealing's resampling rule in host code (mcq_resample_plan_host) against the NumPy / Python-int restatement of
tests/population_util.py, its properties, every refusal, and the layout of the mcq_resample block."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

import mcq_amd
from tests import population_util as pu

abi = mcq_amd.abi
pop = mcq_amd.population
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIN = {"type": "linear_annealing", "beta_start": 1.0, "beta_end": 3.0}


def test_weight_table_is_the_rule():
    for db in (0.0, 1e-9, 0.02, 0.5, 5.0, 40.0):
        want = pu.table(db)
        got = abi.resample_table(db)
        assert got.dtype == np.uint32 and got[0] == 1 << 24
        np.testing.assert_array_equal(got, want, err_msg=f"dbeta = {db}")
        assert len(got) <= 1 << 16 and (len(got) == 1 << 16 or (got[-1] == 0 and (got[:-1] > 0).all()))
    assert len(abi.resample_table(0.0)) == 1 << 16 and len(abi.resample_table(40.0)) == 2
    with pytest.raises(ValueError, match="does not decrease"):
        abi.resample_table(-1e-3)


def test_host_plan_equals_the_restatement():
    for name, e, R, tab, x in pu.plan_vectors():
        want_p, want_s = pu.plan(e, R, tab, x)
        got_p, got_s = mcq_amd._lib.resample_plan_host(e, R, tab, x)
        np.testing.assert_array_equal(got_p, want_p, err_msg=f"{name}: parents")
        np.testing.assert_array_equal(got_s, want_s, err_msg=f"{name}: distinct parents, W, E_min")
        if name.startswith(("equal energies", "capped table")):
            np.testing.assert_array_equal(got_p, np.arange(len(e)), err_msg=f"{name}: equal weights give the identity")


def test_exact_restatement_returns_what_the_int64_one_did():
    """plan() in uint64 / Python ints against its former int64 self, on every vector that one could describe."""
    for name, e, R, tab, x in pu.plan_vectors():
        want_p, want_s = pu.plan_int64(e, R, tab, x)
        got_p, got_s = pu.plan(e, R, tab, x)
        assert got_p.dtype == want_p.dtype and got_s.dtype == want_s.dtype
        np.testing.assert_array_equal(got_p, want_p, err_msg=f"{name}: parents")
        np.testing.assert_array_equal(got_s, want_s, err_msg=f"{name}: distinct parents, W, E_min")
    # ... and where that one could not go: R W = 2^62 exactly (R = 2^19 chains of full weight) is the identity
    R = 1 << 19
    p, s = pu.plan(np.zeros(R, dtype=np.int32), R, pu.table(0.0), [2**32 - 1])
    assert R * int(s[0, 1]) == 2**62 and (p == np.arange(R)).all() and int(s[0, 0]) == R


def test_host_plan_equals_the_restatement_on_the_wide_vectors():
    """mcq_resample_plan_host on tests/population_util.wide_vector_list(): ragged wavefronts and tiles up to MCQ_MAX_POPULATION, caller's
    tables (W = 0 among them), the whole int32 range, entries up to 2^32.  wide_plans() asserts every vector's condition first."""
    plans = pu.wide_plans()
    assert {v.group for v, _, _ in plans} == set(pu.WIDE_GROUPS) and {v.R for v, _, _ in plans} >= set(pu.WIDE_SIZES)
    assert abi.MAX_POPULATION == max(pu.WIDE_SIZES)
    for v, want_p, want_s in plans:
        got_p, got_s = mcq_amd._lib.resample_plan_host(v.energies, v.R, v.table, v.offsets)
        np.testing.assert_array_equal(got_p, want_p, err_msg=f"{v.name}: parents")
        np.testing.assert_array_equal(got_s, want_s, err_msg=f"{v.name}: distinct parents, W, E_min")
        pu.assert_plan_properties(v.energies, v.R, v.table, got_p, v.name)


def test_vectorised_properties_agree_with_the_walk():
    """Both forms pass the host plan of every existing vector up to R = 1 024, and both refuse the same spoilt plans."""
    for name, e, R, tab, x in pu.plan_vectors():
        if R > 1024:
            continue
        p, _ = mcq_amd._lib.resample_plan_host(e, R, tab, x)
        pu.assert_plan_properties(e, R, tab, p, name)
        pu.assert_plan_properties_walk(e, R, tab, p, name)
        spoilt = []
        if (p != np.arange(len(e))).any():
            spoilt.append(np.arange(len(e), dtype=np.int32))                # the identity where the rule moves something
        spoilt.append(np.concatenate([p[:1], p[:-1]]).astype(np.int32))     # shifted by one slot
        spoilt.append(np.where(np.arange(len(e)) % R == R - 1, p - (p % R), p).astype(np.int32))  # the last slot of a population: not monotone
        for q in spoilt:
            if (q == p).all():
                continue
            verdicts = []
            for check in (pu.assert_plan_properties, pu.assert_plan_properties_walk):
                try:
                    check(e, R, tab, q, name)
                    verdicts.append(None)
                except AssertionError as err:
                    verdicts.append(str(err))
            assert verdicts[0] == verdicts[1], f"{name}: the vectorised check says {verdicts[0]!r}, the walk {verdicts[1]!r}"


def test_plan_properties():
    for name, e, R, tab, x in pu.plan_vectors():
        got_p, got_s = mcq_amd._lib.resample_plan_host(e, R, tab, x)
        pu.assert_plan_properties(e, R, tab, got_p, name)
        assert all(int(got_s[g, 0]) == len(np.unique(got_p[g * R: (g + 1) * R])) for g in range(len(e) // R)), name
    # one chain far below the rest takes (nearly) the whole population
    e = np.full(1024, 400, dtype=np.int32)
    e[100] = 3
    p, s = mcq_amd._lib.resample_plan_host(e, 1024, abi.resample_table(0.02), [7])
    assert (p == 100).sum() > 300 and int(s[0, 2]) == 3


def test_plan_refusals():
    tab, e = abi.resample_table(0.02), np.zeros(64, dtype=np.int32)
    for R, x in ((0, []), (-16, []), (24, []), (48, [1]), (1 << 20, [])):
        with pytest.raises(ValueError):
            mcq_amd._lib.resample_plan_host(e, R, tab, x)
    with pytest.raises(ValueError, match="table_len"):
        mcq_amd._lib.resample_plan_host(e, 64, np.zeros(0, dtype=np.uint32), [1])
    with pytest.raises(ValueError, match="table_len"):
        mcq_amd._lib.resample_plan_host(e, 64, np.ones((1 << 16) + 1, dtype=np.uint32), [1])
    L = mcq_amd._lib.lib()
    r = abi.Resample()
    r.n_chains, r.population, r.state_bytes, r.table_len = 64, 64, 36, 10
    assert L.mcq_resample_plan_host(ctypes.byref(r)) == abi.EINVAL and b"required" in L.mcq_population_last_error()
    # the device entry point refuses before it touches a device: a gather in place, misaligned rows, nothing to do
    r.table = r.offsets = r.energies = r.parent = r.stats = 4096
    r.state_in = r.state_out = 8192
    assert L.mcq_resample_device(ctypes.byref(r), None, 0, None) == abi.EINVAL and b"in place" in L.mcq_population_last_error()
    r.state_bytes, r.state_out = 144, 8192 + 144 * 64 + 8
    assert L.mcq_resample_device(ctypes.byref(r), None, 0, None) == abi.EINVAL and b"aligned" in L.mcq_population_last_error()
    r.state_out = 16384
    assert L.mcq_resample_device(ctypes.byref(r), None, 0, None) == abi.ENOMEM and b"scratch" in L.mcq_population_last_error()
    assert L.mcq_resample_scratch_bytes(ctypes.byref(r)) == 64 * 8
    r.state_in = None
    assert L.mcq_resample_device(ctypes.byref(r), None, 0, None) == abi.EINVAL and b"neither" in L.mcq_population_last_error()
    r.run_best_energy = 4096
    assert L.mcq_resample_device(ctypes.byref(r), None, 0, None) == abi.EINVAL and b"summary fold needs" in L.mcq_population_last_error()


def test_anneal_population_refusals():
    """Every refusal raises ValueError before anything is launched: none of these calls reaches a GPU."""
    seeds = abi.seeds_for(1, 64)
    run = lambda **kw: pop.anneal_population(**{**dict(N=6, n_steps=1000, init_mode="random", schedule_params=LIN, seeds=seeds, resample_every=100), **kw})  # noqa: E731
    with pytest.raises(ValueError, match="does not decrease"):
        run(schedule_params={"type": "linear_annealing", "beta_start": 3.0, "beta_end": 1.0})
    with pytest.raises(ValueError, match="does not decrease"):
        run(schedule_params={"type": "sinusoidal_annealing", "beta_start": 3.0, "beta_end": 1.0})
    for s in (0, -5):
        with pytest.raises(ValueError, match="resample_every"):
            run(resample_every=s)
    with pytest.raises(ValueError, match="row limit"):
        run(n_steps=1 << 25, resample_every=1 << 24, trace=True)
    for R in (24, 48, 8, 0):  # no multiple of 16, no divisor of 64, ...
        with pytest.raises(ValueError, match="population"):
            run(population=R)
    with pytest.raises(ValueError, match="2\\^19"):
        run(seeds=abi.seeds_for(0, 1 << 20), population=1 << 20)
    with pytest.raises(ValueError, match="2\\^19"):
        run(seeds=abi.seeds_for(0, 1 << 20))
    with pytest.raises(ValueError, match="multiple of 16"):
        run(seeds=abi.seeds_for(0, 40))
    with pytest.raises(ValueError, match="Philox"):
        pop.check(abi.make_params(6, 1000, "random", LIN, 64, mcmc_type="board", rng="philox"), 100)
    for patience in (0, 500, 1000):  # a board patience that could trigger
        with pytest.raises(ValueError, match="early stopping"):
            pop.check(abi.make_params(6, 1000, "random", LIN, 64, mcmc_type="board", early_stop_patience=patience), 100)
    with pytest.raises(ValueError, match="schedule sets"):
        run(schedule_params=[LIN, LIN])
    p = abi.make_params_sets(6, 1000, "random", [LIN, LIN], 32, mcmc_type="board")
    with pytest.raises(ValueError, match="schedule sets"):
        pop.check(p, 100)
    p = abi.set_exchange(abi.make_params(6, 1000, "random", LIN, 64, mcmc_type="board"), 10, [1.0, 0.9, 0.8, 0.7])
    with pytest.raises(ValueError, match="replica exchange"):
        pop.check(p, 100)
    assert pop.check(abi.make_params(6, 1000, "random", LIN, 64, mcmc_type="board"), 100) == (100, 64)
    assert pop.check(abi.make_params(6, 1000, "random", LIN, 64, mcmc_type="board", early_stop_patience=1001), 100, 16) == (100, 16)
    with pytest.raises(ValueError, match="does not decrease"):
        mcq_amd.drivers.run_competition(N=6, n_runs=64, n_steps=1000, beta_start=3.0, beta_end=1.0, resample_every=100)
    with pytest.raises(ValueError, match="resample_every"):
        mcq_amd.experiments.run_population(6, 1000, "random", None, 64, 0, schedule_params=LIN, mcmc_type="board")


def test_boundaries_of_a_run():
    b = pop.boundaries(LIN, 1050, 100, 2, resample_seed=5)
    assert b["lengths"] == [100] * 10 + [50] and b["offsets"].shape == (10, 2) and b["offsets"].dtype == np.uint32
    np.testing.assert_array_equal(b["offsets"], np.random.RandomState(5).randint(0, 2**32, size=(10, 2), dtype=np.uint32))
    beta = abi.beta_values(LIN, 1050)
    for k in range(10):
        assert b["dbeta"][k] == beta[(k + 1) * 100] - beta[k * 100]
        o, n = int(b["table_off"][k]), int(b["table_len"][k])
        np.testing.assert_array_equal(b["tables"][o: o + n], pu.table(b["dbeta"][k]))
    c = pop.boundaries({"type": "constant", "beta_const": 2.0}, 1000, 100, 1)
    assert len(c["tables"]) == 1 << 16 and (c["table_off"] == 0).all(), "boundaries of equal dbeta share one table"
    assert pop.boundaries(LIN, 100, 100, 1)["lengths"] == [100] and pop.boundaries(LIN, 100, 100, 1)["offsets"].shape == (0, 1)
    np.testing.assert_array_equal(pop.ancestors_of(np.array([[0, 0, 2, 2], [1, 1, 1, 3]], dtype=np.int32), 4), [0, 0, 0, 2])


def test_resample_struct_layout_and_build():
    fields = [f for f, _ in abi.Resample._fields_]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "mcq.h"\nint main(){printf("%zu %d %d %d", sizeof(mcq_resample), MCQ_MAX_POPULATION, MCQ_MAX_RESAMPLE_TABLE, ' \
        "MCQ_RESAMPLE_WEIGHT_BITS);" + "".join(f'printf(" %zu", offsetof(mcq_resample, {f}));' for f in fields) + "return 0;}"
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(prog)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")], check=True)
        out = subprocess.run([os.path.join(d, "t")], capture_output=True, text=True, check=True).stdout.split()
    assert int(out[0]) == ctypes.sizeof(abi.Resample)
    assert [int(x) for x in out[1:4]] == [abi.MAX_POPULATION, abi.MAX_RESAMPLE_TABLE, abi.RESAMPLE_WEIGHT_BITS]
    assert [int(x) for x in out[4:]] == [getattr(abi.Resample, f).offset for f in fields]
    L = mcq_amd._lib.lib()
    assert L.mcq_abi_version() == 6 == abi.ABI_VERSION
    assert os.path.join(mcq_amd.build.CSRC, "mcq_population.hip") in mcq_amd.build.SOURCES
    for name in ("mcq_resample_device", "mcq_resample_plan_host", "mcq_resample_scratch_bytes", "mcq_population_last_error"):
        assert hasattr(L, name), name
