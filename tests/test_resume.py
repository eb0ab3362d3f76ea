"""GPU: chains that run in segments (mcq_run_host_from / mcq_run_device_from / mcq_checkpoint_device through experiments.start_chains,
continue_chains, warm_start_chains) against the reference's chains, against NumPy's own stream, and against the unbroken run on the GPU.
Everything is bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest

import mcq_amd
from tests import resume_util as ru
from tests import util

abi = mcq_amd.abi
ex = mcq_amd.experiments
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AWKWARD = (1, 15, 16, 17, 64)


def _golden_in_segments(golden, case, lanes, cuts, stream_state=None):
    n = case["n_steps"]
    lengths = ru.cuts_to_lengths(cuts, n)
    seed = 0 if stream_state is not None else case["seed"]

    def first(k):
        return ex.start_chains(case["N"], k, case["init"], case["schedule"], [seed], schedule_steps=n, mcmc_type=case["mode"], Q=case.get("Q"),
                               lanes_per_chain=lanes, stream_states=None if stream_state is None else stream_state[None, :])

    res, ckpt = first(lengths[0])
    segs, start = [res], (stream_state if stream_state is not None else seed)
    what = f"G={lanes} cuts={cuts} {case}"
    for i, k in enumerate(lengths):
        if i:
            prev_final = segs[-1]["final_energy"].copy()
            res, ckpt = ex.continue_chains(ckpt, k, lanes_per_chain=lanes)
            np.testing.assert_array_equal(res["initial_energy"], prev_final, err_msg=f"{what}: recounted energy of segment {i}")
            segs.append(res)
        assert int(segs[-1]["near_ties"].sum()) == 0, f"{what}: near tie in segment {i}"
        ru.assert_stream_is_numpys(ckpt.stream_state[0], start, int(ckpt.stream_words[0]), f"{what}: after segment {i}")
    whole = ru.stitch(segs, lengths, ckpt)
    util.assert_chain_equals_golden(whole, 0, case, golden.chain(case), what)


def _seeded_cuts(case, count):
    rs = np.random.RandomState(case["n_steps"] * 131 + case["N"])
    return sorted(int(c) for c in rs.randint(1, max(2, case["n_steps"]), size=count))


def _pick(cases, **want):
    out = [c for c in cases if c.get("patience") is None and c["n_steps"] >= 100 and all(c[k] == v for k, v in want.items())]
    assert out, want
    return out


def test_golden_chains_in_segments(golden):
    """The reference's own chains, run in 2 and in 5 segments: boards at 4 / 8 / 16 / 2 lanes, full_3d slim (4 lanes, N = 9..12) and 8 lanes."""
    picks = []
    for N, lanes in ((3, 4), (6, 4), (12, 4), (12, 2), (12, 8), (12, 16), (6, 2), (17, 8), (24, 8), (20, 16)):
        cs = _pick(golden.chains, mode="board", N=N)
        picks += [(cs[0], lanes), (cs[len(cs) // 2], lanes), (cs[-1], lanes)]
    for N, lanes in ((3, 8), (6, 8), (6, 4), (6, 16), (12, 4), (12, 8), (9, 4), (10, 4), (11, 4), (16, 8)):
        cs = [c for c in golden.chains if c["mode"] == "full_3d" and c["N"] == N and c["n_steps"] >= 100]
        if cs:
            picks += [(cs[0], lanes), (cs[-1], lanes)]
    assert any(c["mode"] == "full_3d" and 9 <= c["N"] <= 12 and lanes == 4 for c, lanes in picks), "no slim full_3d chain among the fixtures"
    for case, lanes in picks:
        n = case["n_steps"]
        _golden_in_segments(golden, case, lanes, [AWKWARD[(n + lanes) % len(AWKWARD)]])           # 2 segments, an awkward cut
        _golden_in_segments(golden, case, lanes, [n - 1])                                           # ... and the last step alone
        _golden_in_segments(golden, case, lanes, [1, 16, 17] + _seeded_cuts(case, 1))               # 5 segments
    case = _pick(golden.chains, mode="board", N=12, n_steps=20000)[0]
    _golden_in_segments(golden, case, 4, [15, 64] + _seeded_cuts(case, 2))


def test_golden_big_wide_q_and_stream_chains_in_segments(golden):
    """Boards beyond N = 32, full_3d beyond N = 32, Q != N^2, and chains whose first segment continues a NumPy stream (stream_states)."""
    for case in golden.chains_big:
        if case.get("patience") is None:
            _golden_in_segments(golden, case, 0, [17])
            _golden_in_segments(golden, case, 8, [1, 15, 16] + _seeded_cuts(case, 1))
    for case in golden.chains_wide[::2]:
        _golden_in_segments(golden, case, 0, [16])
        _golden_in_segments(golden, case, 16, [1, 17, 64] + _seeded_cuts(case, 1))
    for case in golden.chains_q[::3]:
        _golden_in_segments(golden, case, 8, [15])
        _golden_in_segments(golden, case, 0, [1, 16, 64] + _seeded_cuts(case, 1))
    for case in golden.chains_stream[::2]:
        state, _ = golden.stream_state(case)
        _golden_in_segments(golden, case, 0, [17], stream_state=state)
        _golden_in_segments(golden, case, 0, [1, 15, 64] + _seeded_cuts(case, 1), stream_state=state)


# (mode, N, steps of the first segment, seed, words the chain has then taken, NumPy's position): found with the CPU oracle's stream_words
# (constant beta 1.5, random init): positions in the first 16 words of a generation, in its last 48, and exactly at its end -- where the
# sweep has (or has not) run ahead into the next generation when the segment ends
POSITION_CASES = (("board", 6, 400, 100, 2507, 11), ("board", 6, 400, 265, 2490, 618), ("board", 6, 395, 120, 2496, 624),
                  ("full_3d", 6, 37, 104, 637, 13), ("full_3d", 6, 37, 100, 617, 617), ("full_3d", 6, 37, 123, 624, 624))


@pytest.mark.parametrize("mode,N,k,seed,words,pos", POSITION_CASES)
def test_checkpointed_stream_is_numpys_at_the_generation_boundary(mode, N, k, seed, words, pos):
    sp = {"type": "constant", "beta_const": 1.5}
    for lanes in (0, 8, 16):
        res, ckpt = ex.start_chains(N, k, "random", sp, [seed], schedule_steps=k + 300, mcmc_type=mode, lanes_per_chain=lanes)
        assert int(ckpt.stream_words[0]) == words and int(ckpt.stream_state[0, 624]) == pos, (lanes, int(ckpt.stream_words[0]), int(ckpt.stream_state[0, 624]))
        ru.assert_stream_is_numpys(ckpt.stream_state[0], seed, words, f"{mode} N={N} seed={seed} G={lanes}")
        res2, ckpt = ex.continue_chains(ckpt, 300, lanes_per_chain=lanes)
        ru.assert_stream_is_numpys(ckpt.stream_state[0], seed, int(ckpt.stream_words[0]), f"{mode} N={N} seed={seed} G={lanes}, second segment")
        whole, _ = ex.run_chains(N, k + 300, "random", sp, [seed], mcmc_type=mode, lanes_per_chain=lanes)
        util.assert_results_equal(ru.stitch([res, res2], [k, 300], ckpt), whole, f"{mode} N={N} seed={seed} G={lanes}")


def _unbroken_vs_segments(N, mode, sp, n_chains, total, lengths, trace=True, lanes=0, sets=None, init="random", init_modes=None):
    seeds = abi.seeds_for(77, n_chains)
    if sets is None:
        p = abi.make_params(N, total, init, sp, n_chains, mcmc_type=mode, trace=trace, lanes_per_chain=lanes)
        first = lambda k: ex.start_chains(N, k, init, sp, seeds, schedule_steps=total, mcmc_type=mode, trace=trace, lanes_per_chain=lanes)  # noqa: E731
    else:
        cps = n_chains // len(sets)
        p = abi.make_params_sets(N, total, init, sets, cps, mcmc_type=mode, trace=trace, lanes_per_chain=lanes, init_modes=init_modes)
        first = lambda k: ex.start_chains(N, k, init, None, seeds, schedule_steps=total, mcmc_type=mode, trace=trace, lanes_per_chain=lanes,  # noqa: E731
                                          schedule_sets=sets, chains_per_set=cps, init_modes=init_modes)
    whole, _ = mcq_amd._lib.run_host(p, seeds, trace=trace)
    segs, ckpt = ru.run_in_segments(lengths, first, trace=trace, lanes_per_chain=lanes)
    got = ru.stitch(segs, lengths, ckpt, trace=trace)
    what = f"{mode} N={N} {lengths} trace={trace}"
    util.assert_results_equal(got, whole, what, trace=trace is True)
    assert int(np.sum(got["near_ties"])) == int(np.sum(whole["near_ties"])), what
    if trace == "reduced":
        for k in ("step_sum", "step_sumsq", "step_accepted", "step_count"):
            np.testing.assert_array_equal(got[k], whole[k], err_msg=f"{what}: {k}")
    for r in (0, n_chains // 2, n_chains - 1):
        ru.assert_stream_is_numpys(ckpt.stream_state[r], int(seeds[r]), int(ckpt.stream_words[r]), f"{what}: chain {r}")


def test_segments_equal_the_unbroken_run():
    lin = {"type": "linear_annealing", "beta_start": 0.5, "beta_end": 3.0}
    sin = {"type": "sinusoidal_annealing", "beta_start": 0.3, "beta_end": 4.0}
    exp = {"type": "exponential_annealing", "beta_start": 0.5, "beta_end": 5.0}
    log = {"type": "logarithmic_annealing", "beta_start": 0.5, "beta_end": 3.0}
    _unbroken_vs_segments(12, "board", lin, 1030, 3000, [1000, 1, 999, 1000])
    _unbroken_vs_segments(24, "board", sin, 1024, 2000, [700, 17, 1283], trace="reduced")
    _unbroken_vs_segments(12, "full_3d", exp, 1024, 2000, [15, 985, 1000])
    _unbroken_vs_segments(12, "board", log, 1024, 3000, [1500, 1500], trace=False)
    sets = [lin, {"type": "constant", "beta_const": 2.0}, sin, exp]
    _unbroken_vs_segments(11, "board", None, 1024, 1500, [64, 436, 1000], sets=sets, init_modes=["klarner", "random", "latin", "random"])
    _unbroken_vs_segments(10, "full_3d", None, 1024, 1200, [600, 600], sets=sets, init_modes=["latin", "random", "klarner", "random"], trace="reduced")


def test_device_resident_segments_equal_the_host_buffer_path():
    """mcq_run_device_from / mcq_checkpoint_device with torch tensors on one stream: three segments, no host copy of state or stream in between."""
    import torch

    sp = {"type": "exponential_annealing", "beta_start": 0.5, "beta_end": 4.0}
    for mode, N in (("board", 12), ("full_3d", 12)):
        n_chains, k, total = 2048, 700, 2100
        seeds = abi.seeds_for(5, n_chains)
        p = abi.make_params(N, k, "random", sp, n_chains, mcmc_type=mode)
        run = mcq_amd._lib.DeviceRun(p, seeds, schedule_steps=total)
        st = torch.cuda.current_stream()
        host, ckpt = ex.start_chains(N, k, "random", sp, seeds, schedule_steps=total, mcmc_type=mode)
        state = stream_state = None
        for i in range(3):
            run.launch_from(i * k, state=state, stream_state=stream_state, stream=st)
            stream_state = run.checkpoint(stream_state, stream=st)
            state = run.t["final_state"]  # (in place, as include/mcq.h allows: the restore kernel has read it before the same launch's sweep writes it)
            if i:
                host, ckpt = ex.continue_chains(ckpt, k)
            st.synchronize()
            dev = run.results()
            util.assert_results_equal(dev, host, f"{mode} segment {i}: device-resident vs host buffers")
            np.testing.assert_array_equal(stream_state.cpu().numpy().view(np.uint32), host["stream_state"], err_msg=f"{mode} segment {i}: stream")


def test_warm_start_equals_the_draw_free_inits(golden):
    """init = latin, and Klarner where it is exact (gcd(N, 210) = 1), take no initialisation draw: the run equals a warm start from that
    placement with the same seeds, and the recounted initial energy is the analytic value."""
    sp = {"type": "linear_annealing", "beta_start": 0.5, "beta_end": 3.0}
    an = golden.manifest["analytic"]
    for mode in ("board", "full_3d"):
        for init, N in (("latin", 12), ("klarner", 11), ("klarner", 13), ("latin", 7)):
            seeds = abi.seeds_for(300 + N, 64)
            cold, _ = ex.run_chains(N, 1500, init, sp, seeds, mcmc_type=mode)
            i, j = np.meshgrid(np.arange(N), np.arange(N), indexing="ij")
            k = (i + j) % N if init == "latin" else (3 * i + 5 * j) % N
            row = k.ravel() if mode == "board" else np.stack([i.ravel(), j.ravel(), k.ravel()], axis=1).ravel()
            warm, ckpt = ex.warm_start_chains(N, np.tile(row.astype(np.uint8), (64, 1)), seeds, 1500, sp, mcmc_type=mode)
            util.assert_results_equal(warm, cold, f"{mode} {init} N={N}: warm start vs the init kernel")
            want = an["latin_board" if mode == "board" else "latin_full_3d"][str(N)] if init == "latin" else an["klarner_exact_board"][str(N)] if mode == "board" else 0
            assert (warm["initial_energy"] == want).all(), (mode, init, N, warm["initial_energy"][:4], want)
            assert ckpt.step == 1500 and (ckpt.stream_words == warm["stream_words"]).all()


def test_restore_kernel_recounts_random_states():
    rs = np.random.RandomState(99)
    sp = {"type": "constant", "beta_const": 1.0}
    for mode, N, Q in (("board", 5, None), ("board", 12, None), ("board", 33, None), ("board", 128, None), ("full_3d", 4, None), ("full_3d", 12, None),
                       ("full_3d", 7, 100), ("full_3d", 40, None), ("full_3d", 64, 300)):
        n = 6
        if mode == "board":
            states = rs.randint(0, N, size=(n, N * N)).astype(np.uint8)
        else:
            q = Q or N * N
            states = np.stack([np.stack(np.unravel_index(rs.choice(N**3, q, replace=False), (N, N, N)), axis=1).ravel() for _ in range(n)]).astype(np.uint8)
        res, _ = ex.warm_start_chains(N, states, abi.seeds_for(1, n), 0, sp, mcmc_type=mode, Q=Q)
        want = [ru.recount(mode, N, states[r]) for r in range(n)]
        assert res["initial_energy"].tolist() == want and res["final_energy"].tolist() == want, (mode, N, Q)
        np.testing.assert_array_equal(res["final_state"], states)


def test_out_of_range_states_are_clamped():
    """A `state` that is no placement: heights / coordinates beyond the board are clamped to N - 1 (include/mcq.h), nothing else is touched."""
    sp = {"type": "constant", "beta_const": 1.0}
    bad = np.full((4, 36), 255, dtype=np.uint8)
    res, _ = ex.warm_start_chains(6, bad, abi.seeds_for(1, 4), 200, sp, mcmc_type="board")
    ok, _ = ex.warm_start_chains(6, np.full((4, 36), 5, dtype=np.uint8), abi.seeds_for(1, 4), 200, sp, mcmc_type="board")
    util.assert_results_equal(res, ok, "clamped heights")


def test_full_3d_states_that_are_no_placement_and_positions_beyond_624():
    """What include/mcq.h promises for bad input: coordinates beyond the board are clamped to N - 1, two queens on one cell touch nothing but
    the chain's own tables (its energies mean nothing), a stream position above 624 reads as 624."""
    sp = {"type": "constant", "beta_const": 1.0}
    seeds = abi.seeds_for(1, 32)
    for N, lanes in ((6, 8), (12, 4), (12, 8), (40, 16)):
        Q = N * N
        res, _ = ex.warm_start_chains(N, np.full((32, 3 * Q), 255, dtype=np.uint8), seeds, 300, sp, mcmc_type="full_3d", lanes_per_chain=lanes)
        ok, _ = ex.warm_start_chains(N, np.full((32, 3 * Q), N - 1, dtype=np.uint8), seeds, 300, sp, mcmc_type="full_3d", lanes_per_chain=lanes)
        util.assert_results_equal(res, ok, f"full_3d N={N} G={lanes}: clamped coordinates (all queens on one cell)")
        assert res["final_state"].max() <= N - 1
        # a placement with ONE doubled cell runs, and every coordinate it ends on is on the board
        i, j = np.meshgrid(np.arange(N), np.arange(N), indexing="ij")
        row = np.stack([i.ravel(), j.ravel(), ((i + j) % N).ravel()], axis=1)
        row[1] = row[0]
        dup, _ = ex.warm_start_chains(N, np.tile(row.ravel().astype(np.uint8), (32, 1)), seeds, 300, sp, mcmc_type="full_3d", lanes_per_chain=lanes)
        assert dup["final_state"].max() <= N - 1 and (dup["hist_len"] == 301).all()
    p = abi.make_params(6, 200, "random", sp, 32, mcmc_type="board")
    st = np.zeros((32, 36), dtype=np.uint8)
    ss = np.zeros((32, 625), dtype=np.uint32)
    rs = np.random.RandomState(3)
    ss[:, :624] = rs.randint(0, 2**32, size=(32, 624), dtype=np.uint32)
    out = []
    for pos in (624, 625, 1000, 0xFFFFFFFF):
        ss[:, 624] = pos
        out.append(mcq_amd._lib.run_host_from(p, seeds, abi.make_resume(p, 0, 200, state=st, stream_state=ss))[0])
    for o in out[1:]:
        util.assert_results_equal(o, out[0], "a position above 624 reads as 624")
        np.testing.assert_array_equal(o["stream_state"], out[0]["stream_state"])


def test_device_evaluated_beta_of_a_segment():
    """Without a beta_table (a caller that is not this package: _schedules unknown) the device evaluates beta(first_step + s) of the WHOLE
    schedule: segments equal the unbroken run whose beta the device evaluated as well -- all five schedule types, and a schedule set."""
    from mcq_amd.checkpoint import Checkpoint

    scheds = [{"type": "constant", "beta_const": 1.7}, {"type": "linear_annealing", "beta_start": 0.2, "beta_end": 4.0},
              {"type": "exponential_annealing", "beta_start": 0.2, "beta_end": 4.0}, {"type": "logarithmic_annealing", "beta_start": 0.2, "beta_end": 4.0},
              {"type": "sinusoidal_annealing", "beta_start": 0.2, "beta_end": 4.0}]
    total, lengths, n = 1500, [400, 1, 1099], 256
    seeds = abi.seeds_for(9, n)

    def check(make, ckpt_kw, what):
        whole_p = make(total)
        whole_p._schedules = None
        assert abi.host_beta_table(whole_p) is None
        whole, _ = mcq_amd._lib.run_host(whole_p, seeds)
        ckpt = Checkpoint(8, "board", total, seeds, **ckpt_kw)
        segs = []
        for k in lengths:
            p = make(k)
            p._schedules = None
            assert abi.segment_beta_table(p, ckpt.step, total) is None and not p.beta_table
            res, _ = mcq_amd._lib.run_host_from(p, seeds, abi.make_resume(p, ckpt.step, total, state=ckpt.state, stream_state=ckpt.stream_state))
            ckpt.merge(res, k)
            segs.append(res)
        util.assert_results_equal(ru.stitch(segs, lengths, ckpt), whole, what)
        return whole

    runs = [check(lambda k, sp=sp: abi.make_params(8, k, "random", sp, n, mcmc_type="board"), dict(schedule_params=sp), f"device beta, {sp['type']}") for sp in scheds]
    # (the schedules do differ: the check above is not one that any beta passes)
    assert len({r["energy_hist"][:, : total + 1].tobytes() for r in runs}) == len(scheds)
    sets = scheds[1:]
    check(lambda k: abi.make_params_sets(8, k, "random", sets, n // 4, mcmc_type="board"), dict(schedule_sets=sets, chains_per_set=n // 4), "device beta, schedule set")
    # and it is the offset that does it: the second segment evaluated as a schedule of its own differs
    sp = scheds[1]
    p = abi.make_params(8, 400, "random", sp, n, mcmc_type="board")
    p._schedules = None
    first, _ = mcq_amd._lib.run_host_from(p, seeds, abi.make_resume(p, 0, total))
    p2 = abi.make_params(8, 1100, "random", sp, n, mcmc_type="board")
    p2._schedules = None
    right, _ = mcq_amd._lib.run_host_from(p2, seeds, abi.make_resume(p2, 400, total, state=first["final_state"], stream_state=first["stream_state"]))
    wrong, _ = mcq_amd._lib.run_host_from(p2, seeds, abi.make_resume(p2, 0, 1100, state=first["final_state"], stream_state=first["stream_state"]))
    assert not np.array_equal(right["energy_hist"], wrong["energy_hist"])


def test_checkpoint_behind_a_plain_run_with_early_stops_or_exchange():
    """mcq_checkpoint_device behind mcq_run_device: a chain that stopped early stands behind the words of its last step, exchange uniforms
    count like every word -- NumPy's state after stream_words words in both cases."""
    import torch

    sp = {"type": "constant", "beta_const": 3.0}
    seeds = abi.seeds_for(21, 64)
    p1 = abi.make_params(6, 3000, "random", sp, 64, mcmc_type="board", early_stop_patience=40)
    p2 = abi.set_exchange(abi.make_params(12, 1000, "random", sp, 64, mcmc_type="board"), 10, [1.0, 0.9, 0.8, 0.7])
    for p, what in ((p1, "patience"), (p2, "exchange")):
        run = mcq_amd._lib.DeviceRun(p, seeds)
        st = torch.cuda.current_stream()
        run.launch(st)
        ss = run.checkpoint(stream=st)
        st.synchronize()
        res, states = run.results(), ss.cpu().numpy().view(np.uint32)
        if what == "patience":
            assert (res["hist_len"] < 3001).any(), "no chain stopped early"
        for r in range(64):
            ru.assert_stream_is_numpys(states[r], int(seeds[r]), int(res["stream_words"][r]), f"{what}: chain {r}")


def test_a_saved_checkpoint_continues_in_a_fresh_process(tmp_path):
    sp = {"type": "sinusoidal_annealing", "beta_start": 0.3, "beta_end": 4.0}
    seeds = abi.seeds_for(11, 96)
    _, ckpt = ex.start_chains(12, 800, "random", sp, seeds, schedule_steps=2000, mcmc_type="board")
    path, out = str(tmp_path / "ckpt.npz"), str(tmp_path / "seg.npz")
    ckpt.save(path)
    code = ("import sys, numpy as np\nsys.path.insert(0, %r)\nimport mcq_amd\nfrom mcq_amd.checkpoint import Checkpoint\n"
            "c = Checkpoint.load(%r)\nres, c = mcq_amd.experiments.continue_chains(c, 1200)\n"
            "np.savez(%r, ckpt_stream=c.stream_state, best=c.best_energy, stb=c.steps_to_best, **{k: v for k, v in res.items() if isinstance(v, np.ndarray)})\n"
            % (ROOT, path, out))
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT, timeout=600)
    here, ckpt = ex.continue_chains(ckpt, 1200)
    with np.load(out) as z:
        util.assert_results_equal({k: z[k] for k in z.files}, here, "fresh process vs in-process")
        np.testing.assert_array_equal(z["ckpt_stream"], ckpt.stream_state)
        np.testing.assert_array_equal(z["stream_state"], here["stream_state"])
        np.testing.assert_array_equal(z["best"], ckpt.best_energy)
        np.testing.assert_array_equal(z["stb"], ckpt.steps_to_best)


def test_run_experiment_in_segments(golden):
    pl = golden.manifest["plumbing"]
    kw = dict(N=pl["N"], n_steps=pl["n_steps"], init_mode=pl["init"], beta_schedule=None, n_runs=pl["n_runs"], base_seed=pl["base_seed"],
              schedule_params=pl["schedule"], mcmc_type=pl["mode"], early_stop_patience=None)
    a = ex.run_experiment(**kw)
    b = ex.run_experiment(segment_steps=3001, **kw)
    assert a[1] == b[1] == pl["best"] and a[5] == b[5] == pl["steps_to_best"]
    for r in range(pl["n_runs"]):
        np.testing.assert_array_equal(a[0][r], b[0][r])
        np.testing.assert_array_equal(a[3][r], b[3][r])
        np.testing.assert_array_equal(a[4][r], b[4][r])
    with pytest.raises(ValueError, match="early stopping"):
        ex.run_experiment(segment_steps=3001, **dict(kw, early_stop_patience=100))


def test_a_full_trace_past_the_row_limit():
    """One launch refuses a full trace of 2^24 steps; in segments it runs.  Its first 2^22 + 1 entries equal a direct run of that length under
    the whole schedule's beta, and the merged best is the minimum of the history."""
    n_steps, seg = (1 << 24) + 1000, 1 << 22
    sp = {"type": "linear_annealing", "beta_start": 0.2, "beta_end": 2.0}
    with pytest.raises(ValueError):
        ex.run_experiment(6, n_steps, "random", None, 2, base_seed=3, schedule_params=sp, mcmc_type="board", early_stop_patience=None, return_steps=False)
    hist, best, _, _, _, stb = ex.run_experiment(6, n_steps, "random", None, 2, base_seed=3, schedule_params=sp, mcmc_type="board",
                                                  early_stop_patience=None, return_steps=False, segment_steps=seg)
    direct, _ = ex.start_chains(6, seg, "random", sp, abi.seeds_for(3, 2), schedule_steps=n_steps, mcmc_type="board", states=False)
    for r in range(2):
        assert len(hist[r]) == n_steps + 1
        np.testing.assert_array_equal(hist[r][: seg + 1], direct["energy_hist"][r, : seg + 1])
        assert best[r] == int(hist[r].min()) and stb[r] == int(np.argmin(hist[r]))
