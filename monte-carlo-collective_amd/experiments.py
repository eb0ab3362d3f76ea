"""Drop-in for the sweep path of the reference's experiments.py.

Same entry points, argument meaning, return shapes and error behaviour as the reference
(cited per function), but every chain of a call runs in ONE launch of the HIP kernels in
csrc/ through the C-ABI of include/mcq.h -- there is no process pool and no CPU path.

    from mcq_amd.experiments import run_experiment, build_schedule_from_params
"""
import time

import numpy as np

from . import _lib, abi
from .checkpoint import Checkpoint


# --------------------------------------------------------------------------------------------
# beta schedules (experiments.py:13-105).  The reference returns closures; these are callable
# objects that also carry the picklable `params` dict the GPU path consumes.  Their __call__
# evaluates the same float64 expressions on the host (for plots / inspection); the sweep itself
# evaluates beta on the device.
# --------------------------------------------------------------------------------------------
class BetaSchedule:
    def __init__(self, params, n_steps):
        self.params = dict(params)
        self.n_steps = int(n_steps)

    def __call__(self, step):
        t, n = self.params["type"], self.n_steps
        if t == "constant":
            return self.params["beta_const"]
        bs, be = self.params["beta_start"], self.params["beta_end"]
        if n <= 1:
            return be
        if t == "linear_annealing":
            frac = step / (n - 1)
            return bs + frac * (be - bs)
        if t == "exponential_annealing":
            s = min(max(step, 0), n - 1)
            return bs * np.exp(np.log(be / bs) * (s / (n - 1)))
        if t == "logarithmic_annealing":
            s = min(max(step, 0), n)
            return bs + (be - bs) * (np.log(1 + s) / np.log(1 + n))
        s = min(max(step, 0), n)
        return bs + (be - bs) * (1 - np.cos(np.pi * s / n)) / 2

    def __repr__(self):
        return f"BetaSchedule({self.params}, n_steps={self.n_steps})"


def constant_beta(beta):
    return BetaSchedule({"type": "constant", "beta_const": beta}, 0)


def linear_annealing_beta(beta_start, beta_end, n_steps):
    return BetaSchedule({"type": "linear_annealing", "beta_start": beta_start, "beta_end": beta_end}, n_steps)


def exponential_annealing_beta(beta_start, beta_end, n_steps):
    return BetaSchedule({"type": "exponential_annealing", "beta_start": beta_start, "beta_end": beta_end}, n_steps)


def logarithmic_annealing_beta(beta_start, beta_end, n_steps):
    return BetaSchedule({"type": "logarithmic_annealing", "beta_start": beta_start, "beta_end": beta_end}, n_steps)


def sinusoidal_annealing_beta(beta_start, beta_end, n_steps):
    return BetaSchedule({"type": "sinusoidal_annealing", "beta_start": beta_start, "beta_end": beta_end}, n_steps)


def build_schedule_from_params(sched_type, n_steps, beta_const=None, beta_start=None, beta_end=None):
    """experiments.py:79-105, including its ValueErrors."""
    if sched_type == "constant":
        if beta_const is None:
            raise ValueError("beta_const required for constant schedule")
        return BetaSchedule({"type": "constant", "beta_const": beta_const}, n_steps)
    if sched_type in ("linear_annealing", "exponential_annealing", "logarithmic_annealing", "sinusoidal_annealing"):
        if beta_start is None or beta_end is None:
            raise ValueError(f"beta_start and beta_end required for {sched_type} schedule")
        return BetaSchedule({"type": sched_type, "beta_start": beta_start, "beta_end": beta_end}, n_steps)
    raise ValueError(f"Unknown betta_scheduling type: {sched_type}")


_DESC = {
    "linear_annealing": ("linear beta: {s}->{e}", "Linear {s}->{e}"),
    "exponential_annealing": ("exp beta: {s}->{e}", "Exponential {s}->{e}"),
    "logarithmic_annealing": ("log beta: {s}->{e}", "Logarithmic {s}->{e}"),
    "sinusoidal_annealing": ("sinusoidal beta: {s}->{e}", "Sinusoidal {s}->{e}"),
}


def _describe(sched_type, beta_const, beta_start, beta_end):
    if sched_type == "constant":
        return {"type": "constant", "beta_const": beta_const}, f"constant beta={beta_const}", f"Constant beta={beta_const}"
    if sched_type in _DESC:
        d, l = _DESC[sched_type]
        return ({"type": sched_type, "beta_start": beta_start, "beta_end": beta_end},
                d.format(s=beta_start, e=beta_end), l.format(s=beta_start, e=beta_end))
    raise ValueError(f"Unknown betta_scheduling type: {sched_type}")


def build_schedule_from_common(common_cfg, n_steps):
    """experiments.py:108-152: common['betta_scheduling'] -> (schedule, base_seed, desc, schedule_params)."""
    cfg = common_cfg["betta_scheduling"]
    st = cfg["type"]
    base_seed = cfg.get("base_seed", 0)
    if st == "constant":
        params, desc, _ = _describe(st, cfg["beta_const"], None, None)
    elif st in _DESC:
        params, desc, _ = _describe(st, None, cfg["beta_start"], cfg["beta_end"])
    else:
        raise ValueError(f"Unknown betta_scheduling type: {st}")
    sched = build_schedule_from_params(st, n_steps, params.get("beta_const"), params.get("beta_start"), params.get("beta_end"))
    return sched, base_seed, desc, params


def build_schedules_from_types(sched_types, sched_cfg, n_steps):
    """experiments.py:155-196: requires base_seed, beta_start, beta_end and beta_const keys."""
    base_seed = sched_cfg["base_seed"]
    beta_start, beta_end, beta_const = sched_cfg["beta_start"], sched_cfg["beta_end"], sched_cfg["beta_const"]
    out = []
    for st in sched_types:
        params, desc, label = _describe(st, beta_const, beta_start, beta_end)
        sched = build_schedule_from_params(st, n_steps, params.get("beta_const"), params.get("beta_start"), params.get("beta_end"))
        out.append((sched, base_seed, desc, label, params))
    return out


# --------------------------------------------------------------------------------------------
# states handed back to callers (competition.py:179-187 reads best_state.heights)
# --------------------------------------------------------------------------------------------
class BoardState:
    """Stand-in for State3DQueensBoard: N, Q and the heights array (mcmc_board.py:23-28)."""

    def __init__(self, N, heights, energy):
        self.N, self.Q = N, N * N
        self.heights = np.asarray(heights, dtype=np.int64).reshape(N, N)
        self._energy = int(energy)

    def energy(self, recompute=False):
        return self._energy


class QueensState:
    """Stand-in for State3DQueens: N, Q, queens[Q,3] and the occupied-cell set (mcmc.py:15-18, 101, 113-118)."""

    def __init__(self, N, queens, energy):
        self.queens = np.asarray(queens, dtype=np.int64).reshape(-1, 3)
        self.N, self.Q = N, len(self.queens)
        self.occ_set = {tuple(int(v) for v in q) for q in self.queens}
        self._energy = int(energy)

    def energy(self, recompute=False):
        return self._energy


def _state(mode, N, row, energy):
    return BoardState(N, row, energy) if mode == abi.MODE_BOARD else QueensState(N, row, energy)


# --------------------------------------------------------------------------------------------
# the sweep
# --------------------------------------------------------------------------------------------
def run_chains(N, n_steps, init_mode, schedule_params, seeds, mcmc_type="full_3d", early_stop_patience=None,
               trace=True, states=True, flags=0, lanes_per_chain=0, Q=None, stream_states=None):
    """Lowest Python level: every chain of `seeds` in one GPU launch.  `stream_states` (one np.random.get_state() tuple or uint32[625] row per
    chain): the chains continue those MT19937 streams instead of seeding their own; `stream_words` of the result says how far each went.

    Returns (result dict of NumPy arrays as described in include/mcq.h, kernel seconds)."""
    seeds = np.asarray(seeds)
    params = abi.make_params(N, n_steps, init_mode, schedule_params, len(seeds), mcmc_type=mcmc_type,
                             early_stop_patience=early_stop_patience, trace=trace, flags=flags,
                             lanes_per_chain=lanes_per_chain, Q=Q)
    if stream_states is not None:
        abi.set_stream_states(params, stream_states)
    if seeds.size and (seeds.min() < 0 or seeds.max() > 2**32 - 1):
        raise ValueError("Seed must be between 0 and 2**32 - 1")
    return _lib.run_host(params, seeds.astype(np.uint32), trace=trace, states=states)


# --------------------------------------------------------------------------------------------
# chains in segments: the concatenation of the segments IS the unbroken run, bit for bit (include/mcq.h: mcq_resume)
# --------------------------------------------------------------------------------------------
def _run_segment(ckpt, n_steps, state, stream_state, trace, states, lanes_per_chain, flags, init_mode="random", init_modes=None,
                 first_stream_states=None):
    n_steps = int(n_steps)
    if n_steps < 0 or ckpt.step + n_steps > ckpt.schedule_steps:
        raise ValueError(f"a segment of {n_steps} steps from step {ckpt.step} leaves the schedule of {ckpt.schedule_steps} steps")
    p = ckpt.params(n_steps, trace=trace, lanes_per_chain=lanes_per_chain, flags=flags, init_mode=init_mode, init_modes=init_modes)
    if first_stream_states is not None:
        abi.set_stream_states(p, first_stream_states)
    r = abi.make_resume(p, ckpt.step, ckpt.schedule_steps, state=state, stream_state=stream_state)
    res, secs = _lib.run_host_from(p, ckpt.seeds, r, checkpoint=True, trace=trace, states=True)
    ckpt.merge(res, n_steps)
    if not states:
        res.pop("best_state"), res.pop("final_state")
    res["kernel_seconds"] = secs
    return res, ckpt


def start_chains(N, n_steps, init_mode, schedule_params, seeds, schedule_steps=None, mcmc_type="full_3d", trace=True, states=True,
                 flags=0, lanes_per_chain=0, Q=None, stream_states=None, schedule_sets=None, chains_per_set=None, init_modes=None):
    """The first `n_steps` steps of chains whose schedule is `schedule_steps` long (default: n_steps): like run_chains, but beta follows the
    WHOLE schedule and the chains can go on (continue_chains).  Early stopping is off.  `schedule_sets` / `chains_per_set` / `init_modes`
    run several schedules side by side (abi.make_params_sets; `schedule_params` is then unused).

    Returns (result dict of the segment -- every field relative to the segment, plus `stream_state` and `kernel_seconds` --, Checkpoint)."""
    seeds = np.asarray(seeds)
    if seeds.size and (seeds.min() < 0 or seeds.max() > 2**32 - 1):
        raise ValueError("Seed must be between 0 and 2**32 - 1")
    total = int(n_steps) if schedule_steps is None else int(schedule_steps)
    ckpt = Checkpoint(N, mcmc_type, total, seeds.astype(np.uint32), schedule_params=None if schedule_sets is not None else schedule_params,
                      schedule_sets=schedule_sets, chains_per_set=chains_per_set, Q=Q, trace=trace)
    return _run_segment(ckpt, n_steps, None, None, trace, states, lanes_per_chain, flags, init_mode=init_mode, init_modes=init_modes,
                        first_stream_states=stream_states)


def continue_chains(ckpt, n_steps, trace=None, states=True, lanes_per_chain=0, flags=0, N=None, mcmc_type=None, Q=None):
    """The next `n_steps` steps of the chains of `ckpt` (which is updated and returned): steps [ckpt.step, ckpt.step + n_steps) of the
    schedule, from the checkpoint's placements and streams.  `trace` defaults to the checkpoint's.  N / mcmc_type / Q, when given, must
    be the checkpoint's (ValueError otherwise).  Returns (result dict of the segment, ckpt)."""
    ckpt.require(N=N, mcmc_type=mcmc_type, Q=Q)
    if ckpt.state is None or ckpt.stream_state is None:
        raise ValueError("the checkpoint holds no placements / streams to continue from")
    return _run_segment(ckpt, n_steps, ckpt.state, ckpt.stream_state, ckpt.trace if trace is None else trace, states, lanes_per_chain, flags)


def warm_start_chains(N, states_in, seeds, n_steps, schedule_params, schedule_steps=None, mcmc_type="full_3d", trace=True, states=True,
                      flags=0, lanes_per_chain=0, Q=None, schedule_sets=None, chains_per_set=None):
    """Chains that start from GIVEN placements (`states_in`: uint8[n_chains][state_bytes] in the final_state layout -- N*N heights, or
    (i, j, k) per queen), e.g. a known good board to be polished: seeded with `seeds` like any chain, no initialisation draw taken --
    which is what the reference's latin and exact-Klarner inits do.  Returns (result dict, Checkpoint) like start_chains."""
    seeds = np.asarray(seeds)
    if seeds.size and (seeds.min() < 0 or seeds.max() > 2**32 - 1):
        raise ValueError("Seed must be between 0 and 2**32 - 1")
    total = int(n_steps) if schedule_steps is None else int(schedule_steps)
    ckpt = Checkpoint(N, mcmc_type, total, seeds.astype(np.uint32), schedule_params=None if schedule_sets is not None else schedule_params,
                      schedule_sets=schedule_sets, chains_per_set=chains_per_set, Q=Q, trace=trace)
    return _run_segment(ckpt, n_steps, np.asarray(states_in, dtype=np.uint8), None, trace, states, lanes_per_chain, flags)


def accepted_rejected_steps(res, r):
    """Step indices of accepted / rejected proposals of chain r (experiments.py:329-332)."""
    n = int(res["steps_executed"][r])
    bits = np.unpackbits(res["accept_bits"][r].view(np.uint8), bitorder="little")[:n].astype(bool)
    idx = np.arange(n)
    return idx[bits], idx[~bits]


def _chain_dict(res, r, mode, N):
    """The dict metropolis_mcmc[_board] returns (experiments.py:270-279, 367-376)."""
    L = int(res["hist_len"][r])
    acc, rej = accepted_rejected_steps(res, r)
    return {
        "final_state": _state(mode, N, res["final_state"][r], res["final_energy"][r]),
        "final_energy": int(res["final_energy"][r]),
        "best_state": _state(mode, N, res["best_state"][r], res["best_energy"][r]),
        "best_energy": int(res["best_energy"][r]),
        "energy_history": res["energy_hist"][r, :L],
        "accepted_steps": acc,
        "rejected_steps": rej,
        "steps_to_best": int(res["steps_to_best"][r]),
    }


def _params_of(beta_schedule, schedule_params):
    if schedule_params is not None:
        return schedule_params
    p = getattr(beta_schedule, "params", None)
    if p is None:
        raise ValueError("the GPU path needs schedule_params (or a schedule built by build_schedule_from_params)")
    return p


def _one_chain(seed, **kw):
    """One chain, seeded (np.random.seed(seed), experiments.py:200-201, 287-288) or -- seed=None, the reference's default -- drawn from NumPy's
    global stream where it stands: the chain runs on the device from a copy of np.random.get_state(), and the global stream is then moved past
    the words the chain took (mcq_outputs.stream_words), so whatever draws from it next sees what it would see after the reference's call."""
    if seed is not None:
        return run_chains(seeds=[seed], **kw)[0]
    st = np.random.get_state()
    res, _ = run_chains(seeds=[0], stream_states=st, **kw)
    left = int(res["stream_words"][0])
    while left > 0:  # RandomState.randint over the full 32-bit range takes exactly one word per element
        n = min(left, 1 << 24)
        np.random.randint(0, 2**32, size=n, dtype=np.uint32)
        left -= n
    return res


def metropolis_mcmc_board(N, n_steps, init_mode, beta_schedule, verbose=True, seed=None, run_idx=None,
                          early_stop_patience=None, schedule_params=None):
    """experiments.py:282-376 for one chain; seed=None continues NumPy's global stream like the reference (_one_chain)."""
    res = _one_chain(seed, N=N, n_steps=n_steps, init_mode=init_mode, schedule_params=_params_of(beta_schedule, schedule_params), mcmc_type="board",
                     early_stop_patience=early_stop_patience)
    d = _chain_dict(res, 0, abi.MODE_BOARD, N)
    if verbose and n_steps > 0:
        print(d["final_energy"])
        print(d["best_energy"])
    return d


def metropolis_mcmc(N, n_steps, init_mode, beta_schedule, verbose=True, seed=None, Q=None, run_idx=None,
                    early_stop_patience=None, schedule_params=None):
    """experiments.py:199-279 for one chain; early_stop_patience is accepted and ignored, as there; seed=None continues NumPy's global stream."""
    res = _one_chain(seed, N=N, n_steps=n_steps, init_mode=init_mode, schedule_params=_params_of(beta_schedule, schedule_params), mcmc_type="full_3d", Q=Q)
    d = _chain_dict(res, 0, abi.MODE_FULL3D, N)
    if verbose and n_steps > 0:
        print(d["final_energy"])
        print(d["best_energy"])
    return d


def run_single_chain(N, n_steps, init_mode, beta_schedule, seed=None, verbose=False, run_idx=None, early_stop_patience=None):
    """experiments.py:379-389"""
    return metropolis_mcmc(N=N, n_steps=n_steps, init_mode=init_mode, beta_schedule=beta_schedule, verbose=verbose,
                           seed=seed, run_idx=run_idx, early_stop_patience=early_stop_patience)


def run_single_chain_board(N, n_steps, init_mode, beta_schedule, seed=None, verbose=False, run_idx=None, early_stop_patience=None):
    """experiments.py:392-402"""
    return metropolis_mcmc_board(N=N, n_steps=n_steps, init_mode=init_mode, beta_schedule=beta_schedule, verbose=verbose,
                                 seed=seed, run_idx=run_idx, early_stop_patience=early_stop_patience)


def _multithread(args, board):
    (N, n_steps, init_mode, schedule_params, seed, verbose, run_idx, early_stop_patience) = args
    sched = build_schedule_from_params(schedule_params["type"], n_steps, schedule_params.get("beta_const"),
                                       schedule_params.get("beta_start"), schedule_params.get("beta_end"))
    t0 = time.time()
    fn = run_single_chain_board if board else run_single_chain
    res = fn(N=N, n_steps=n_steps, init_mode=init_mode, beta_schedule=sched, seed=seed, verbose=verbose, run_idx=run_idx,
             early_stop_patience=early_stop_patience)
    return {"run_idx": run_idx, "best_state": res["best_state"], "energy_history": res["energy_history"],
            "best_energy": res["best_energy"], "duration": time.time() - t0, "accepted_steps": res["accepted_steps"],
            "rejected_steps": res["rejected_steps"], "steps_to_best": res["steps_to_best"]}


def run_single_chain_multithread(args):
    """experiments.py:405-437"""
    return _multithread(args, board=False)


def run_single_chain_board_multithread(args):
    """experiments.py:440-472"""
    return _multithread(args, board=True)


def run_experiment(N, n_steps, init_mode, beta_schedule, n_runs, base_seed=0, verbose=False, n_workers=None,
                   schedule_params=None, mcmc_type="full_3d", early_stop_patience=100000, return_steps=True,
                   lanes_per_chain=0, segment_steps=None):
    """experiments.py:475-573.  Chain r is seeded with base_seed + r and results come back ordered by r.

    Returns the reference's 6-tuple (all_histories, best_energies, run_times, all_accepted_steps,
    all_rejected_steps, all_steps_to_best); histories and step lists are NumPy arrays (one per chain,
    ragged after an early stop), which every consumer in the reference accepts
    (np.array(histories), len(histories[0]), list.extend).  `n_workers` is accepted and unused: all
    chains run in one kernel launch.  With return_steps=False the two step-index lists are empty
    (they are O(n_runs * n_steps) on the host).

    Reference behaviours kept: n_runs > 1 requires schedule_params (experiments.py:505-506);
    n_runs == 1 drops early_stop_patience (experiments.py:550-558); full_3d ignores it.

    segment_steps (not in the reference; default None = one launch): the chains run in segments of at most that many steps
    (start_chains / continue_chains), the traces are stitched on the host and the same 6-tuple comes back, bit for bit what one
    launch gives -- and a full trace of 2^24 steps and more, which one launch refuses, becomes possible for callers with the host
    memory for it.  A board patience that could trigger cannot be carried across segments: pass early_stop_patience=None."""
    if n_runs > 1:
        if schedule_params is None:
            raise ValueError("schedule_params is required for parallel execution when n_runs > 1")
        patience = early_stop_patience
    else:
        schedule_params = _params_of(beta_schedule, schedule_params) if n_runs == 1 else schedule_params
        patience = None
    if n_runs <= 0:
        return [], [], [], [], [], []
    seeds = abi.seeds_for(base_seed, n_runs)
    if segment_steps is not None:
        return _run_experiment_segments(N, int(n_steps), init_mode, schedule_params, seeds, mcmc_type, patience, return_steps, lanes_per_chain,
                                        int(segment_steps), verbose)
    res, secs = run_chains(N, n_steps, init_mode, schedule_params, seeds, mcmc_type=mcmc_type, early_stop_patience=patience,
                           states=False, lanes_per_chain=lanes_per_chain)
    all_histories = [res["energy_hist"][r, : int(res["hist_len"][r])] for r in range(n_runs)]
    best_energies = [int(b) for b in res["best_energy"]]
    run_times = [secs / n_runs] * n_runs
    all_acc, all_rej = [], []
    if return_steps:
        for r in range(n_runs):
            a, j = accepted_rejected_steps(res, r)
            all_acc.append(a)
            all_rej.append(j)
    else:
        all_acc, all_rej = [[] for _ in range(n_runs)], [[] for _ in range(n_runs)]
    all_steps_to_best = [int(s) for s in res["steps_to_best"]]
    if verbose:
        for b in best_energies:
            print(b)
    return all_histories, best_energies, run_times, all_acc, all_rej, all_steps_to_best


def _run_experiment_segments(N, n_steps, init_mode, schedule_params, seeds, mcmc_type, patience, return_steps, lanes_per_chain, segment_steps, verbose):
    """run_experiment(..., segment_steps=...): the same chains in segments, stitched."""
    if segment_steps <= 0 or abi.hist_stride_for(segment_steps) >= abi.MAX_HIST_STRIDE:
        raise ValueError(f"segment_steps must be positive and leave a trace row below 2^24 entries, got {segment_steps}")
    if abi.mode_of(mcmc_type) == abi.MODE_BOARD and abi.normalise_patience(patience) >= 0 and abi.normalise_patience(patience) <= n_steps:
        raise ValueError("early stopping that could trigger cannot be carried across segments: pass early_stop_patience=None")
    n_runs = len(seeds)
    hist = [np.empty(n_steps + 1, dtype=np.int32) for _ in range(n_runs)]
    acc = [[] for _ in range(n_runs)]
    rej = [[] for _ in range(n_runs)]
    secs, done, ckpt = 0.0, 0, None
    while True:
        n = min(segment_steps, n_steps - done)
        if ckpt is None:
            res, ckpt = start_chains(N, n, init_mode, schedule_params, seeds, schedule_steps=n_steps, mcmc_type=mcmc_type, states=False,
                                     lanes_per_chain=lanes_per_chain)
        else:
            res, ckpt = continue_chains(ckpt, n, states=False, lanes_per_chain=lanes_per_chain)
        secs += res["kernel_seconds"]
        for r in range(n_runs):
            if done == 0:
                hist[r][: n + 1] = res["energy_hist"][r, : n + 1]
            else:  # entry 0 of a later segment repeats the last entry of the one before
                hist[r][done + 1: done + n + 1] = res["energy_hist"][r, 1: n + 1]
            if return_steps:
                a, j = accepted_rejected_steps(res, r)
                acc[r].append(a + done), rej[r].append(j + done)
        done += n
        if done >= n_steps:
            break
    best_energies = [int(b) for b in ckpt.best_energy]
    if return_steps:
        all_acc, all_rej = [np.concatenate(a) for a in acc], [np.concatenate(j) for j in rej]
    else:
        all_acc, all_rej = [[] for _ in range(n_runs)], [[] for _ in range(n_runs)]
    if verbose:
        for b in best_energies:
            print(b)
    return hist, best_energies, [secs / n_runs] * n_runs, all_acc, all_rej, [int(s) for s in ckpt.steps_to_best]


def run_population(N, n_steps, init_mode, beta_schedule, n_runs, resample_every, population=None, resample_seed=0, base_seed=0, verbose=False,
                   schedule_params=None, mcmc_type="full_3d", return_steps=True, lanes_per_chain=0, quench=False):
    """run_experiment's 6-tuple over population annealing (population.anneal_population; not in the reference): the n_runs chains, seeded
    base_seed + r, are resampled every `resample_every` steps inside populations of `population` chains (None: one population of all).
    Run r of the result is SLOT r: its history is the slot's own, joined the way run_experiment(segment_steps=) joins segments, so it
    may jump at a boundary where the slot took over a parent's placement.  There is no early stopping: it cannot be carried across segments.
    quench=True (boards only; off by default): every slot's best placement is quenched to a local minimum on the device behind the run
    (population.anneal_population(quench=True)) and the tuple gains a SEVENTH element, a dict of `quenched_state`, `quenched_energy` and
    `quench_moves`; the six elements before it are what the call without it returns."""
    from . import population as _pop

    if n_runs <= 0:
        return [], [], [], [], [], []
    sp = _params_of(beta_schedule, schedule_params)
    seeds = abi.seeds_for(base_seed, n_runs)
    timings = {}
    res, _ = _pop.anneal_population(N, n_steps, init_mode, sp, seeds, resample_every, population=population, resample_seed=resample_seed,
                                    mcmc_type=mcmc_type, trace=True, states=False, lanes_per_chain=lanes_per_chain, timings=timings, quench=quench)
    all_histories = [res["energy_hist"][r, : int(n_steps) + 1] for r in range(n_runs)]
    best_energies = [int(b) for b in res["best_energy"]]
    if return_steps:
        pairs = [accepted_rejected_steps(res, r) for r in range(n_runs)]
        all_acc, all_rej = [a for a, _ in pairs], [j for _, j in pairs]
    else:
        all_acc, all_rej = [[] for _ in range(n_runs)], [[] for _ in range(n_runs)]
    if verbose:
        for b in best_energies:
            print(b)
    six = (all_histories, best_energies, [timings["run_seconds"] / n_runs] * n_runs, all_acc, all_rej, [int(s) for s in res["steps_to_best"]])
    if quench:
        return six + ({k: res[k] for k in ("quenched_state", "quenched_energy", "quench_moves")},)
    return six
