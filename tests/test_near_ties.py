"""GPU: the sweep kernel's accept decision and near-tie counter on beta tables crafted to put the uniform next to exp(-beta dE)
(tests/near_tie_util.py; the oracle's side is pinned on the CPU by tests/test_near_ties_host.py), the same through chains in segments,
and the population fold kernel on summaries that tie, wrap and pass 2^31.  Everything is bit for bit.

ASSUMPTION of the tie points: the device's float64 exp and glibc's agree within 1 ulp at the crafted arguments.  The ties stand 2 or 3 ulp
from the uniform, so with that agreement the count (|distance| <= 4) and the decision (the sign) are certain; the near misses stand at 8.
Nobody has measured the agreement elsewhere: these points are the only test of it.  A crafted step that decides or counts differently on
the device is first of all a measurement of a disagreement of 2 ulp or more at that argument (profiles/near_ties.md), not yet a kernel bug."""
import numpy as np
import pytest

import mcq_amd
from oracle import oracle
from tests import near_tie_util as nt
from tests import population_util as pu
from tests import resume_util as ru
from tests import util

abi = mcq_amd.abi
pytestmark = pytest.mark.gpu
NAMES = [c.name for c in nt.CASES]
REDUCED_FIELDS = ("step_sum", "step_sumsq", "step_accepted", "step_count")
_oracle_runs = {}


def _oracle(case, table):
    """The oracle's run of a case under its crafted table: computed once, shared, left unchanged.  For a reduced-trace case it is the run
    with the full trace plus the per-set sums of that trace."""
    if case.name not in _oracle_runs:
        reduced = case.trace == "reduced"
        res = oracle.run(case.params(table, trace=True if reduced else "case"), case.seeds(), trace=True if reduced else case.trace, n_threads=8)
        if reduced:
            res.update(nt.reduced_from_trace(res, case.n_steps, case.n_sets))
        _oracle_runs[case.name] = res
    return _oracle_runs[case.name]


def _assert_equal(got, want, case, points, what):
    """Every field of util.RESULT_FIELDS (near_ties among them), histories and accept bits or the reduced trace; a failure names the first
    differing (chain, step) and says whether it was crafted."""
    try:
        assert "near_ties" in util.RESULT_FIELDS
        util.assert_results_equal(got, want, what, trace=case.trace is True)
        np.testing.assert_array_equal(got["near_ties"], want["near_ties"], err_msg=f"{what}: near_ties per chain")
        if case.trace == "reduced":
            for k in REDUCED_FIELDS:
                np.testing.assert_array_equal(got[k], want[k], err_msg=f"{what}: {k}")
    except AssertionError as e:
        raise AssertionError(f"{e}\n{what}: {nt.first_difference(got, want, points, trace=case.trace)}") from None


def sweep_equals_the_oracle_next_to_exp(name, row=None):
    """Bracketed and with MCQ_FLAG_EXACT_EXP: both runs are the oracle's, tie for tie.  `row` (tests/test_philox_ties.py): the row of
    SWEEP_TABLE the launch must take, as (MODE, G, PATIENCE, NT, REDUCED, NC), on the stream the case names."""
    case = nt.CASES_BY_NAME[name]
    table, points = nt.crafted(name)
    nt.check_plan_was_met(case, points)
    seeds, crafted = case.seeds(), nt.expected_near_ties(case, points)
    want = _oracle(case, table)
    np.testing.assert_array_equal(want["near_ties"], crafted, err_msg=f"{name}: the oracle's own count (tests/test_near_ties_host.py)")
    v = mcq_amd._lib.sweep_variant(case.params(table))
    assert v["PATIENCE"] == (case.patience is not None) and v["REDUCED"] == (case.trace == "reduced")
    assert v["SLIM"] == (name == "full3d10_g4") and v["WIDE"] == (name == "full3d40") and (not case.lanes or v["G"] == case.lanes)
    assert v["PHILOX"] == (case.rng == "philox") and not v["EXCH"]
    assert row is None or tuple(int(v[k]) for k in ("MODE", "G", "PATIENCE", "NT", "REDUCED", "NC")) == row, (name, v)
    for flags, how in ((0, "bracketed"), (abi.FLAG_EXACT_EXP, "exact exp")):
        got, _ = mcq_amd._lib.run_host(case.params(table, flags=flags), seeds, trace=case.trace)
        total = int(got["near_ties"].sum())
        _assert_equal(got, want, case, points, f"{name} {how}")
        assert total != 0 and total == int(crafted.sum()), f"{name} {how}: {total} near ties, {int(crafted.sum())} crafted"
        np.testing.assert_array_equal(got["near_ties"], crafted, err_msg=f"{name} {how}: near ties per chain vs the crafted counts")
        if case.trace is True:
            for pt in points:
                if pt["kind"] != "behind":
                    assert nt.accept_bit(got, pt["chain"], pt["step"]) == int(pt["accept"]), (name, how, pt)


@pytest.mark.parametrize("name", NAMES)
def test_sweep_equals_the_oracle_next_to_exp(name):
    sweep_equals_the_oracle_next_to_exp(name)


def _cuts_around_a_tie(case, points):
    """One cut directly before and one directly after a crafted tie (two different ties, so that there are three segments)."""
    ties = sorted({pt["step"] for pt in points if pt["counts"]})
    a, b = ties[len(ties) // 3], ties[2 * len(ties) // 3]
    assert 0 < a and a + 1 < b + 1 < case.n_steps
    return [a, b + 1 - a, case.n_steps - (b + 1)], a, b


@pytest.mark.parametrize("name", nt.SEGMENT_CASES)
def test_segments_add_the_near_ties_up(name):
    """Three segments through _lib.run_host_from, each under its slice of the crafted table, cut directly before one tie and directly
    after another: Checkpoint.merge and resume_util.stitch give the unbroken run's near ties per chain, and the rest as in test_resume."""
    case = nt.CASES_BY_NAME[name]
    table, points = nt.crafted(name)
    seeds, crafted = case.seeds(), nt.expected_near_ties(case, points)
    lengths, a, b = _cuts_around_a_tie(case, points)
    whole, _ = mcq_amd._lib.run_host(case.params(table), seeds)
    ckpt = mcq_amd.checkpoint.Checkpoint(case.N, case.mode, case.n_steps, seeds, schedule_sets=case.base_schedules(), chains_per_set=case.set_chains)
    segs = []
    for k in lengths:
        p = case.params(table, n_steps=k, first_step=ckpt.step)
        r = abi.make_resume(p, ckpt.step, case.n_steps, state=ckpt.state, stream_state=ckpt.stream_state)
        res, _ = mcq_amd._lib.run_host_from(p, seeds, r)
        in_segment = np.zeros(case.n_chains, dtype=np.int64)
        for pt in points:
            if ckpt.step <= pt["step"] < ckpt.step + k:
                in_segment[pt["chain"]] += pt["counts"]
        np.testing.assert_array_equal(res["near_ties"], in_segment, err_msg=f"{name}: near ties of steps [{ckpt.step}, {ckpt.step + k})")
        ckpt.merge(res, k)
        segs.append(res)
    assert all(int(s["near_ties"].sum()) > 0 for s in segs), f"{name}: a segment without a tie: {lengths}"
    got = ru.stitch(segs, lengths, ckpt)
    what = f"{name} in segments {lengths} (cuts before the tie of step {a} and after the tie of step {b})"
    _assert_equal(got, whole, case, points, what)
    _assert_equal(got, _oracle(case, table), case, points, what + " vs the oracle")
    assert int(crafted.sum()) > 0
    np.testing.assert_array_equal(ckpt.near_ties, crafted, err_msg=f"{what}: Checkpoint.merge")
    np.testing.assert_array_equal(got["near_ties"], crafted, err_msg=f"{what}: stitched")
    np.testing.assert_array_equal(whole["near_ties"], crafted, err_msg=f"{what}: the unbroken run")
    for r in (0, case.n_chains // 2, case.n_chains - 1):
        ru.assert_stream_is_numpys(ckpt.stream_state[r], int(seeds[r]), int(ckpt.stream_words[r]), f"{what}: chain {r}")


# ---- the fold kernel of population annealing (mcq_resample_device with state_in == NULL) ---------------------------------------------

GUARD, fold_rule, fold_vectors, _guarded = pu.GUARD, pu.fold_rule, pu.fold_vectors, pu.guarded  # (shared with tests/test_population.py)


def _fold_on_device(first_step, seg, run, state_bytes, optional=("near_ties", "stream_words", "best_state"), half=None):
    """One mcq_resample_device call that only folds.  Returns the run's arrays afterwards; every array, given or not, sits between guard
    bytes that are checked.  half = (name, "seg" | "run"): that side of an optional pair is left out (the call must refuse)."""
    import torch

    dev = torch.device("cuda", torch.cuda.current_device())
    st = torch.cuda.current_stream(dev)
    n = len(seg["best_energy"])
    bufs = {(side, k): _guarded(torch, dev, d[k]) for side, d in (("seg", seg), ("run", run)) for k in d}
    r = abi.Resample()
    r.n_chains, r.population, r.state_bytes, r.first_step = n, 16, state_bytes, int(first_step)
    for (side, k), (_, view) in bufs.items():
        if k in optional or k in ("best_energy", "steps_to_best", "n_accepted"):
            if half != (k, side):
                setattr(r, f"{side}_{k}", view.data_ptr())
    scratch = torch.empty(8, dtype=torch.uint8, device=dev)
    before = {key: buf.cpu().numpy().copy() for key, (buf, _) in bufs.items()}
    mcq_amd._lib.resample_device(r, scratch, st)
    st.synchronize()
    out = {}
    for (side, k), (buf, view) in bufs.items():
        now = buf.cpu().numpy()
        assert (now[:64] == GUARD).all() and (now[-64:] == GUARD).all(), f"guard bytes around {side}_{k} were written"
        given = k in optional or k in ("best_energy", "steps_to_best", "n_accepted")
        if side == "seg" or not given:
            np.testing.assert_array_equal(now, before[(side, k)], err_msg=f"{side}_{k} must not be written")
        if side == "run":
            out[k] = now[64:-64].view(run[k].dtype).reshape(run[k].shape).copy()
    return out


@pytest.mark.parametrize("first_step", (0, 5000, 2**31 + 12345))
@pytest.mark.parametrize("state_bytes", (36, 81, 144))
def test_fold_kernel_equals_the_merge_rule(first_step, state_bytes):
    """4096 slots; rows of 36, 81 and 144 bytes move 4, 1 and 16 bytes at a time.  first_step == 0 overwrites the garbage in run_*."""
    seg, run, counts = fold_vectors(first_step, state_bytes, seed=first_step % 1000 + state_bytes)
    assert counts["seg_ties"] >= 700 and counts["run_ties"] >= 700 and counts["both_ties"] >= 300 and counts["wraps"] >= 500
    assert counts["equal"] >= 500 and counts["lower"] >= 500 and counts["far_steps"] >= 500
    want = fold_rule(first_step, seg, run)
    if first_step:
        eq, lo = seg["best_energy"] == run["best_energy"], seg["best_energy"] < run["best_energy"]
        assert (want["steps_to_best"][eq] == run["steps_to_best"][eq]).all() and (want["best_state"][eq] == run["best_state"][eq]).all()
        assert (want["steps_to_best"][lo] == first_step + seg["steps_to_best"][lo]).all() and (want["best_state"][lo] == seg["best_state"][lo]).all()
        assert int((want["steps_to_best"] > 2**31).sum()) >= 500 and int((want["near_ties"] > 2**32).sum()) > 0
    else:
        assert all((want[k] == seg[k]).all() for k in want)
    got = _fold_on_device(first_step, seg, run, state_bytes)
    for k in want:
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"first_step {first_step}: run_{k} after the fold")


@pytest.mark.parametrize("optional", ((), ("near_ties",), ("stream_words",), ("best_state",)))
def test_fold_kernel_leaves_absent_pairs_alone(optional):
    """With optional pairs absent the fold still follows the rule on the rest, and neither those arrays nor any guard byte is written."""
    seg, run, _ = fold_vectors(777, 36, seed=11)
    want = fold_rule(777, seg, {k: v for k, v in run.items() if k in optional or k in ("best_energy", "steps_to_best", "n_accepted")})
    got = _fold_on_device(777, seg, run, 36, optional=optional)
    for k in run:
        np.testing.assert_array_equal(got[k], want[k] if k in want else run[k], err_msg=f"optional {optional}: run_{k}")


def test_fold_refuses_half_given_pairs():
    seg, run, _ = fold_vectors(777, 36, seed=12)
    for k in ("near_ties", "stream_words", "best_state"):
        for side in ("seg", "run"):
            with pytest.raises(ValueError, match="both the segment's and the run's"):
                _fold_on_device(777, seg, run, 36, half=(k, side))
