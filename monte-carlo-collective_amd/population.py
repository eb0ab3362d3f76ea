"""Population annealing: chains that are resampled between device segments (include/mcq.h: mcq_resample, csrc/mcq_population.hip).

NOT a mode of the reference -- its chains never learn from each other --, never a default, and labelled as such like Philox and
replica exchange.  A run of n_steps steps under one beta schedule is cut into segments of `resample_every` steps; at every inner
boundary the chains of a population are resampled on the device in proportion to exp(-dbeta E): slot m takes the placement (and with
it the energy) of a parent of its population and keeps its own random stream, its own history and its own running best.  The rule is
integer-exact (include/mcq.h), so a NumPy restatement equals the kernel bit for bit (tests/population_util.py).

Everything between the first launch and the last stays on the device and on one stream: mcq_run_device_from -> mcq_checkpoint_device
-> mcq_resample_device per segment.  Only a full trace (trace=True) is copied to the host segment by segment.
"""
import ctypes as C

import numpy as np

from . import _lib, abi


def check(params, resample_every, population=None, trace=False):
    """What population annealing does not run, as ValueError before anything is launched: `params` is the Params block of the WHOLE run.
    Returns (S, R): the segment length and the population size in force."""
    n, n_steps = int(params.n_chains), int(params.n_steps)
    S = int(resample_every)
    if S <= 0:
        raise ValueError(f"resample_every must be positive, got {resample_every}")
    if n_steps < 1:
        raise ValueError("population annealing needs at least one step")
    if params.n_sets > 1:
        raise ValueError("population annealing runs one schedule: schedule sets are not resampled")
    if params.rng != abi.RNG_MT19937_NUMPY:
        raise ValueError("population annealing continues MT19937 streams across segments: Philox is not served")
    if params.exchange_every > 0:
        raise ValueError("population annealing and replica exchange do not combine (the rungs are not part of a checkpoint)")
    if params.mode == abi.MODE_BOARD and 0 <= params.patience <= n_steps:
        raise ValueError("early stopping that could trigger cannot be carried across segments: pass early_stop_patience=None")
    if trace is True and abi.hist_stride_for(min(S, n_steps)) >= abi.MAX_HIST_STRIDE:
        raise ValueError(f"a full trace of segments of {min(S, n_steps)} steps reaches the row limit of 2^24 entries: resample more often, or trace='reduced'")
    R = n if population is None else int(population)
    if R <= 0 or R % 16 or R > abi.MAX_POPULATION:
        raise ValueError(f"a population is a positive multiple of 16 chains, at most 2^19, got {R}")
    if n % R:
        raise ValueError(f"the population ({R}) must divide the number of chains ({n})")
    return S, R


def boundaries(schedule_params, n_steps, resample_every, n_populations, resample_seed=0):
    """The host half of the rule (include/mcq.h, steps 1, 2 and 4) for a run of n_steps steps cut every `resample_every`:
    returns a dict with the segment `lengths` (K entries), `dbeta` float64[K - 1], the weight `tables` of all boundaries in one uint32
    array with `table_off` / `table_len` per boundary (boundaries of equal dbeta share one table), and the offset words
    `offsets` uint32[K - 1][n_populations].  ValueError for a schedule that decreases over a segment."""
    n_steps, S = int(n_steps), int(resample_every)
    K = -(-n_steps // S)
    lengths = [S] * (K - 1) + [n_steps - (K - 1) * S]
    beta = abi.beta_values(schedule_params, n_steps)
    at = np.arange(K, dtype=np.int64) * S
    dbeta = beta[at[1:]] - beta[at[:-1]]
    if (dbeta < 0).any() or not np.isfinite(dbeta).all():
        k = int(np.flatnonzero(~(dbeta >= 0))[0]) + 1
        raise ValueError(f"population annealing needs a schedule that does not decrease: beta({k * S}) - beta({(k - 1) * S}) = {float(dbeta[k - 1])}")
    parts, where, off, ln, total = [], {}, [], [], 0
    for db in dbeta:
        key = float(db)
        if key not in where:
            t = abi.resample_table(key)
            where[key] = (total, len(t))
            parts.append(t)
            total += len(t)
        off.append(where[key][0]), ln.append(where[key][1])
    tables = np.concatenate(parts) if parts else np.zeros(1, dtype=np.uint32)
    offsets = np.random.RandomState(resample_seed).randint(0, 2**32, size=(K - 1, int(n_populations)), dtype=np.uint32)
    return {"lengths": lengths, "dbeta": dbeta, "tables": np.ascontiguousarray(tables, dtype=np.uint32), "table_off": np.array(off, dtype=np.int64),
            "table_len": np.array(ln, dtype=np.int64), "offsets": np.ascontiguousarray(offsets)}


def ancestors_of(parents, n_chains):
    """The segment-0 slot every final placement descends from: the parents of all boundaries composed, int32[n_chains]."""
    anc = np.arange(n_chains, dtype=np.int32)
    for par in parents:
        anc = anc[par]
    return anc


def anneal_population(N, n_steps, init_mode, schedule_params, seeds, resample_every, population=None, resample_seed=0, mcmc_type="board",
                      trace=False, states=True, lanes_per_chain=0, Q=None, timings=None, quench=False):
    """Every chain of `seeds` for n_steps steps, resampled every `resample_every` steps inside populations of `population` consecutive
    chains (None: all chains form one population).

    Returns (res, lineage).  `res` holds, per slot and for the whole run, the fields run_chains returns: initial_energy of the first
    segment, final_energy / final_state of the last, best_energy / best_state / steps_to_best merged over the slot's segments (a later
    segment moves them only by a strictly lower energy; steps_to_best in whole-run steps), the sums of n_accepted, stream_words and
    near_ties, `stream_state` (the MT19937 states after the run), and the trace by mode: trace=False none, "reduced" the per-entry sums
    of the segments joined by dropping each later segment's entry 0, True the same join of the full histories and accept bits (made on
    the host, segment by segment).  Entry 0 of a later segment is the energy of the PARENT's placement, so a slot's history may jump
    at a boundary, and its best_energy may be an energy it received rather than one its history shows.
    `lineage`: `parents` int32[K - 1][n_chains] (chain indices), `distinct_parents`, `weight_sum` and `e_min` int64[K - 1][populations],
    `ancestors` int32[n_chains], and per segment `segment_initial_energy` / `segment_final_energy` int32[K][n_chains] plus
    `received_energy` int32[K - 1][n_chains], the energy each slot took over at a boundary.

    ValueError before anything is launched (check, boundaries): a schedule that decreases over a segment, a resample_every <= 0, a
    population that does not divide the chains, is no multiple of 16 or exceeds 2^19, a full-trace segment row at the 2^24 limit.  The
    chains run NumPy's stream without early stopping or replica exchange; check() refuses a Params block that says otherwise.
    `timings` (a dict, optional) receives wall seconds of the enqueue + wait.
    quench=True (boards only; off by default, and nothing changes when off): best_state of every slot is quenched to a local minimum
    (quench.quench_device) on the same stream behind the last fold, with no host synchronisation before it; `res` gains `quenched_state`
    uint8[n_chains][N*N], `quenched_energy` and `quench_moves` int32[n_chains].  Every other field is what the run without it returns.
    quench="pairs" (boards up to N = 32) takes the pair-move quench instead (quench.quench_pairs_device): the same three fields, and
    `quench_pair_moves`, `quench_rounds`, `quench_certified`, `quench_energy_single` int32[n_chains]."""
    import time

    import torch

    seeds = np.asarray(seeds)
    if seeds.size and (seeds.min() < 0 or seeds.max() > 2**32 - 1):
        raise ValueError("Seed must be between 0 and 2**32 - 1")
    seeds = seeds.astype(np.uint32)
    if isinstance(schedule_params, (list, tuple)):
        raise ValueError("population annealing runs one schedule: schedule sets are not resampled")
    from . import quench as _quench

    _quench.check_mode(quench, N, board=abi.mode_of(mcmc_type) == abi.MODE_BOARD)
    if quench and abi.mode_of(mcmc_type) != abi.MODE_BOARD:
        raise ValueError("quench=True: the quench runs boards only (mcmc_type='board')")
    n = len(seeds)
    mk = lambda steps: abi.make_params(N, steps, init_mode, schedule_params, n, mcmc_type=mcmc_type, early_stop_patience=None, trace=trace,  # noqa: E731
                                       lanes_per_chain=lanes_per_chain, Q=Q)
    whole = mk(n_steps)
    S, R = check(whole, resample_every, population, trace=trace)
    n_steps, pops = int(n_steps), n // R
    b = boundaries(schedule_params, n_steps, S, pops, resample_seed)
    lengths, K = b["lengths"], len(b["lengths"])
    first = 0
    for L in lengths:  # the resume-side refusals (mcq_validate_resume), before anything is launched
        r = abi.Resume()
        r.first_step, r.schedule_steps = first, n_steps
        _lib.validate_resume(mk(L), r)
        first += L
    sb = abi.state_bytes(whole.N, whole.mode, whole.n_queens)

    dev = torch.device("cuda", torch.cuda.current_device())
    st = torch.cuda.current_stream(dev)
    t_start = time.perf_counter()
    with torch.cuda.device(dev), torch.cuda.stream(st):
        runs = {L: _lib.DeviceRun(mk(L), seeds, trace=trace, states=True, schedule_steps=n_steps) for L in sorted(set(lengths), reverse=True)}
        i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)  # noqa: E731
        i64 = lambda *shape: torch.empty(shape, dtype=torch.int64, device=dev)  # noqa: E731
        acc = {"best_energy": i32(n), "steps_to_best": i64(n), "n_accepted": i64(n), "near_ties": i64(n), "stream_words": i32(n),
               "best_state": torch.empty((n, sb), dtype=torch.uint8, device=dev)}
        pop_state = torch.empty((n, sb), dtype=torch.uint8, device=dev)
        seg_e0, seg_e1, received = i32(K, n), i32(K, n), i32(max(K - 1, 1), n)
        parents, stats = i32(max(K - 1, 1), n), i64(max(K - 1, 1), pops, 3)
        # the weight tables and the offset words: uploaded once, before the first launch
        tables = torch.from_numpy(b["tables"].view(np.int32)).to(dev)
        offsets = torch.from_numpy(b["offsets"].view(np.int32).reshape(K - 1, pops).copy()).to(dev) if K > 1 else None
        probe = abi.Resample()
        probe.n_chains = n
        scratch = torch.empty(max(8, int(_lib.lib().mcq_resample_scratch_bytes(C.byref(probe)))), dtype=torch.uint8, device=dev)
        reduced = None
        if trace == "reduced":
            reduced = {k: i64(n_steps + 1) for k in ("step_sum", "step_sumsq", "step_accepted", "step_count")}
        hist = bits = None
        if trace is True:
            hist = np.zeros((n, abi.hist_stride_for(n_steps)), dtype=np.int32)
            bits = np.zeros((n, abi.bits_stride_for(n_steps) * 64), dtype=np.uint8)

        state = stream_state = None
        done = 0
        t_enq = time.perf_counter()
        for k, L in enumerate(lengths):
            run = runs[L]
            run.launch_from(done, state=state, stream_state=stream_state, stream=st)
            stream_state = run.checkpoint(stream_state, stream=st)
            seg_e0[k].copy_(run.t["initial_energy"]), seg_e1[k].copy_(run.t["final_energy"])
            r = abi.Resample()
            r.n_chains, r.population, r.state_bytes, r.first_step = n, R, sb, done
            for f in ("best_energy", "steps_to_best", "n_accepted", "near_ties", "stream_words", "best_state"):
                setattr(r, "seg_" + f, run.t[f].data_ptr()), setattr(r, "run_" + f, acc[f].data_ptr())
            if k < K - 1:
                r.table, r.table_len = tables.data_ptr() + 4 * int(b["table_off"][k]), int(b["table_len"][k])
                r.offsets, r.energies = offsets[k].data_ptr(), run.t["final_energy"].data_ptr()
                r.state_in, r.state_out = run.t["final_state"].data_ptr(), pop_state.data_ptr()  # (the next segment writes final_state again: two buffers)
                r.parent, r.stats, r.energy_out = parents[k].data_ptr(), stats[k].data_ptr(), received[k].data_ptr()
            _lib.resample_device(r, scratch, st)
            if reduced is not None:
                for key, big in reduced.items():
                    if k == 0:
                        big[: L + 1].copy_(run.t[key][: L + 1])
                    else:  # entry 0 of a later segment is the entry before, again -- of the resampled placements
                        big[done + 1: done + L + 1].copy_(run.t[key][1: L + 1])
            if hist is not None:  # a full trace goes to the host segment by segment
                st.synchronize()
                h = run.t["energy_hist"].cpu().numpy()
                if k == 0:
                    hist[:, : L + 1] = h[:, : L + 1]
                else:
                    hist[:, done + 1: done + L + 1] = h[:, 1: L + 1]
                a = np.ascontiguousarray(run.t["accept_bits"].cpu().numpy()).view(np.uint8)
                bits[:, done: done + L] = np.unpackbits(a, axis=1, bitorder="little")[:, :L]
            state = pop_state
            done += L
        quenched = None
        if quench:  # behind the last fold, which has written acc["best_state"]; same stream, nothing waited for
            quenched = _quench.hook_device(N, acc["best_state"], quench, st)
        t_wait = time.perf_counter()
        st.synchronize()
        t_end = time.perf_counter()
    if timings is not None:
        timings.update(setup_seconds=t_enq - t_start, enqueue_seconds=t_wait - t_enq, run_seconds=t_end - t_enq)

    last = runs[lengths[-1]].results()
    u32 = lambda t: t.cpu().numpy().view(np.uint32)  # noqa: E731
    res = {
        "hist_len": np.full(n, n_steps + 1, dtype=np.int64),
        "steps_executed": np.full(n, n_steps, dtype=np.int64),
        "initial_energy": seg_e0[0].cpu().numpy(),
        "final_energy": last["final_energy"],
        "best_energy": acc["best_energy"].cpu().numpy(),
        "steps_to_best": acc["steps_to_best"].cpu().numpy(),
        "n_accepted": acc["n_accepted"].cpu().numpy(),
        "near_ties": acc["near_ties"].cpu().numpy(),
        "stream_words": u32(acc["stream_words"]),
        "stream_state": u32(stream_state),
    }
    if states:
        res["best_state"], res["final_state"] = acc["best_state"].cpu().numpy(), last["final_state"]
    if quenched is not None:
        _quench.hook_results(res, quenched)
    if reduced is not None:
        res.update({key: big.cpu().numpy() for key, big in reduced.items()})
    if hist is not None:
        res["energy_hist"] = hist
        res["accept_bits"] = np.ascontiguousarray(np.packbits(bits, axis=1, bitorder="little")).view(np.uint64)
    par = parents[: K - 1].cpu().numpy()
    sts = stats[: K - 1].cpu().numpy()
    lineage = {"parents": par, "distinct_parents": sts[:, :, 0].copy(), "weight_sum": sts[:, :, 1].copy(), "e_min": sts[:, :, 2].copy(),
               "ancestors": ancestors_of(par, n), "segment_initial_energy": seg_e0.cpu().numpy(), "segment_final_energy": seg_e1.cpu().numpy(),
               "received_energy": received[: K - 1].cpu().numpy(), "lengths": list(lengths), "population": R, "dbeta": b["dbeta"]}
    return res, lineage
