"""Parallel tempering of the board heat-bath sweep, one ladder per workgroup (include/mcq.h: mcq_temper, where the rule is stated;
csrc/mcq_temper.hip).

NOT a mode of the reference, never a default, and labelled as such like Philox, replica exchange in the Metropolis sweep, population
annealing, the quench and the heat bath.  The R = 2, 4, 8 or 16 replicas of a ladder are consecutive chain slots; each runs
heatbath.py's sweep at beta_s times the multiplier of its RUNG, and after every K-th sweep neighbouring rungs are offered a swap of
their temperatures.  Placements, seeds, streams, best values and histories stay with their slots.  The whole run is one launch.  The
rule is integer-exact, so the library's host code, the kernel and a NumPy restatement (tests/temper_util.py) agree bit for bit.

Boards (temper_states*, temper_device): N = 2 .. 32 with every R and N = 33 .. 64 with R = 2 or 4 on the device (a ladder must fit the
LDS of a workgroup), every N = 2 .. 128 in the host code.

full_3d placements have a rule and a kernel of their own (include/mcq.h: mcq_temper3d; csrc/mcq_temper3d.hip): temper_queens,
temper_queens_device, temper_queens_host.  The replicas run heatbath.py's QUEEN sweep, each on an attack field of its own in the LDS
of the ladder's workgroup; the exchange is the same with a stream of its own.  On the device as far as abi.temper3d_lds_bytes stays
within the workgroup's LDS (with Q = N^2: every R to N = 18, R <= 8 to N = 20, R <= 4 to N = 25, R = 2 to N = 32), every N = 2 .. 32 in
the host code.  A ladder in which a slot holds two queens in one cell is handed back unmoved (flags).  anneal_tempered runs either
under a schedule (mcmc_type="board" or "full_3d").

Out of scope for both, and refused or absent rather than approximated: the drivers, jobs.JobSet, the YAML keys and bench.py.
"""
import numpy as np

from . import _lib, abi
from .heatbath import FORMS, _host_seeds, _upload, to_numpy  # noqa: F401  (to_numpy: the dict temper_device returned, as NumPy arrays)
from .quench import _device_out, _device_queens, _device_states, _host_outputs, _host_queens, _host_states, _queens_of

FIELDS = ("state", "energy_in", "energy_out", "best_energy", "best_sweep", "best_state", "n_changed", "rung_out", "n_exchanges", "pair_accepted")
FIELDS_3D = FIELDS + ("flags",)
# FORMS is heatbath.FORMS: the two kernels of the tempered board sweep.  "lines" (mcq_temper_device, every N a ladder fits, the default)
# tests the cells of a column's four lines; "counters" (mcq_temper_counters_device, N <= abi.MAX_N_TEMPER_COUNTERS) reads per-line queen
# counters.  Same rule, same results.


def _check_form(form, N, mcmc_type="board"):
    """ValueError for an unknown form, for the counter form beyond its largest N and for the counter form of full_3d placements; nothing
    here touches the GPU."""
    if form not in FORMS:
        raise ValueError(f"Unknown form {form!r}: the tempered heat-bath sweep of boards has the forms {FORMS}")
    if form == "counters" and mcmc_type == "full_3d":
        raise ValueError(f'the tempered heat-bath queen sweep of full_3d placements has the one form "lines", got form={form!r}')
    if form == "counters" and int(N) > abi.MAX_N_TEMPER_COUNTERS:
        raise ValueError(f'form="counters" runs N <= {abi.MAX_N_TEMPER_COUNTERS}, got N = {int(N)}; form="lines" runs every N a ladder fits')


def _block(N, n, n_sweeps, first_sweep, R, K, table_len, swap_len):
    q = abi.Temper()
    q.N, q.mode, q.n_chains, q.n_sweeps, q.first_sweep = int(N), abi.MODE_BOARD, int(n), int(n_sweeps), int(first_sweep)
    q.replicas, q.exchange_every, q.table_len, q.swap_len = int(R), int(K), int(table_len), int(swap_len)
    q.n_events = abi.temper_events(first_sweep, n_sweeps, K)
    return q


def _block3d(N, Q, n, n_sweeps, first_sweep, R, K, table_len, swap_len):
    q = abi.Temper3D()
    q.N, q.n_queens, q.n_chains, q.n_sweeps, q.first_sweep = int(N), int(Q), int(n), int(n_sweeps), int(first_sweep)
    q.replicas, q.exchange_every, q.table_len, q.swap_len = int(R), int(K), int(table_len), int(swap_len)
    q.n_events = abi.temper_events(first_sweep, n_sweeps, K)
    return q


def _host_rungs(rungs, n):
    r = np.asarray(rungs)
    if r.size and (r.min() < 0 or r.max() > 255):
        raise ValueError("a rung is an integer in 0 .. replicas - 1")
    r = np.ascontiguousarray(r, dtype=np.uint8).reshape(-1)
    if len(r) != n:
        raise ValueError(f"rungs must have one entry per chain: {len(r)} rungs, {n} chains")
    return r


def _host_call(block, run, dtypes, s, seeds, betas, ladder, exchange_every, first_sweep, rungs, trace):
    """What temper_states_host and temper_queens_host share: the seeds and both tables checked, the parameter block from
    block(n_chains, n_sweeps, R, table_len, swap_len), the host outputs and the call `run` of the library."""
    n = s.shape[0]
    seeds = _host_seeds(seeds, n)
    T, X = abi.temper_tables(betas, ladder, exchange_every, first_sweep)
    R, n_sweeps = T.shape[1], int(np.asarray(betas).size)
    q = block(n, n_sweeps, R, T.shape[2], X.shape[2])
    out = _host_outputs(q, s, dtypes, like=("best_state",))
    out["pair_accepted"] = np.zeros((n // R, R - 1), dtype=np.int64)
    q.pair_accepted = out["pair_accepted"].ctypes.data
    q.seeds, q.table, q.swap_table = seeds.ctypes.data, T.ctypes.data, X.ctypes.data if X.shape[0] else None
    if rungs is not None:
        rungs = _host_rungs(rungs, n)
        q.rung_in = rungs.ctypes.data
    if trace:
        out["energy_hist"] = np.zeros((n, n_sweeps + 1), dtype=np.int32)
        out["rung_hist"] = np.zeros((n, n_sweeps + 1), dtype=np.uint8)
        q.energy_hist, q.rung_hist, q.hist_stride = out["energy_hist"].ctypes.data, out["rung_hist"].ctypes.data, n_sweeps + 1
    run(q)
    return out


def temper_states_host(N, states, seeds, betas, ladder, exchange_every=1, first_sweep=0, rungs=None, trace=False):
    """mcq_temper_host: the rule in the library's plain host code, NumPy in and out, no GPU.  Same arguments and result as temper_states."""
    K = exchange_every
    return _host_call(lambda n, n_sweeps, R, D, DX: _block(N, n, n_sweeps, first_sweep, R, K, D, DX), _lib.temper_host, abi.TEMPER_DTYPES,
                      _host_states(N, states), seeds, betas, ladder, K, first_sweep, rungs, trace)


def temper_queens_host(N, states, seeds, betas, ladder, Q=None, exchange_every=1, first_sweep=0, rungs=None, trace=False):
    """mcq_temper3d_host: the full_3d rule in the library's plain host code, NumPy in and out, no GPU.  Same arguments and result as
    temper_queens."""
    K, Qn = exchange_every, _queens_of(N, Q)
    return _host_call(lambda n, n_sweeps, R, D, DX: _block3d(N, Qn, n, n_sweeps, first_sweep, R, K, D, DX), _lib.temper3d_host, abi.TEMPER3D_DTYPES,
                      _host_queens(N, states, Q), seeds, betas, ladder, K, first_sweep, rungs, trace)


def device_tables(betas, ladder, exchange_every=1, first_sweep=0, device=None):
    """abi.temper_tables on the device as two int32 tensors (the uint32 entries bit for bit), uploaded on torch's current stream: what
    temper_device takes as `tables`.  The rows belong to the call they were built for: exchange_every and first_sweep decide which sweep
    an event follows."""
    return _upload_tables(*abi.temper_tables(betas, ladder, exchange_every, first_sweep), device)


def _upload_tables(T, X, device):
    if X.shape[0] == 0:  # no event: one row that no event reads, so that the tensor has an address
        X = np.zeros((1,) + X.shape[1:], dtype=np.uint32)
    return _upload(T.view(np.int32), device), _upload(X.view(np.int32), device)


def _device_call(n, block, run, dtypes, states, seeds, betas, ladder, exchange_every, first_sweep, rungs, tables, out, trace, best_state, stream):
    """What temper_device and temper_queens_device share behind the check of `states`: the tables, seeds and rungs on the device (checked
    when given as tensors, uploaded otherwise), the result tensors, the parameter block from block(n_sweeps, R, table_len, swap_len)
    and the call `run` of the library on the stream."""
    import torch

    dev = states.device
    st = torch.cuda.current_stream(dev) if stream is None else stream
    K = int(exchange_every)
    with torch.cuda.device(dev), torch.cuda.stream(st):
        if tables is not None:
            T, X = tables
            for t, what, cap in ((T, "T [n_sweeps][R][table_len <= 512]", abi.MAX_HEATBATH_TABLE), (X, "X [n_events][R - 1][swap_len <= 4096]", abi.MAX_TEMPER_SWAP_TABLE)):
                if not (isinstance(t, torch.Tensor) and t.dtype == torch.int32 and t.device == dev and t.dim() == 3 and t.is_contiguous() and 1 <= t.shape[2] <= cap):
                    raise ValueError(f"tables on the device are contiguous int32 tensors {what} (device_tables)")
            if int(X.shape[1]) != int(T.shape[1]) - 1:
                raise ValueError(f"tables: X has {int(X.shape[1])} pairs of rungs, T has {int(T.shape[1])} rungs")
            n_sweeps = int(T.shape[0]) if betas is None else int(np.asarray(betas).size)
            if n_sweeps > int(T.shape[0]) or abi.temper_events(first_sweep, n_sweeps, K) > int(X.shape[0]):
                raise ValueError("tables: fewer rows than the call has sweeps or events")
        else:
            if betas is None or ladder is None:
                raise ValueError("a tempered call on the device needs betas and ladder, or tables")
            T, X = device_tables(betas, ladder, K, first_sweep, dev)
            n_sweeps = int(T.shape[0]) if np.asarray(betas).size else 0
        R = int(T.shape[1])
        if isinstance(seeds, torch.Tensor):
            if seeds.dtype != torch.int32 or seeds.device != dev or not seeds.is_contiguous() or tuple(seeds.shape) != (n,):
                raise ValueError("seeds must be a contiguous int32 tensor [n_chains] on the device of states (the uint32 seeds bit for bit)")
        else:
            seeds = _upload(_host_seeds(seeds, n).view(np.int32), dev)
        if rungs is not None:
            if isinstance(rungs, torch.Tensor):
                if rungs.dtype != torch.uint8 or rungs.device != dev or not rungs.is_contiguous() or tuple(rungs.shape) != (n,):
                    raise ValueError("rungs must be a contiguous uint8 tensor [n_chains] on the device of states")
            else:
                rungs = _upload(_host_rungs(rungs, n), dev)
        q = block(n_sweeps, R, T.shape[2], X.shape[2])
        res = {"state": _device_out(out, states)}
        tdt = {np.int32: torch.int32, np.int64: torch.int64, np.uint8: torch.uint8}
        for k, dt in dtypes.items():
            res[k] = torch.empty(n, dtype=tdt[dt], device=dev)
        res["pair_accepted"] = torch.empty((n // R if R and n % R == 0 else 0, R - 1), dtype=torch.int64, device=dev)
        if best_state:
            res["best_state"] = torch.empty_like(states)
        if trace:
            res["energy_hist"] = torch.empty((n, n_sweeps + 1), dtype=torch.int32, device=dev)
            res["rung_hist"] = torch.empty((n, n_sweeps + 1), dtype=torch.uint8, device=dev)
        q.seeds, q.table, q.swap_table = seeds.data_ptr(), T.data_ptr(), X.data_ptr() if q.n_events else None
        q.state_in, q.state_out, q.rung_in = states.data_ptr(), res["state"].data_ptr(), None if rungs is None else rungs.data_ptr()
        for k in tuple(dtypes) + ("pair_accepted", "best_state", "energy_hist", "rung_hist"):
            if k in res and res[k].numel():
                setattr(q, k, res[k].data_ptr())
        q.hist_stride = n_sweeps + 1
        run(q, st)
        for t in (seeds, T, X, rungs):  # (the kernel reads them after this call has returned)
            if t is not None:
                t.record_stream(st)
    return res


def temper_device(N, states, seeds, betas=None, ladder=None, exchange_every=1, first_sweep=0, rungs=None, tables=None, out=None, trace=False,
                  best_state=True, stream=None, form="lines"):
    """mcq_temper_device on a torch uint8 tensor [n_chains][N*N] of the current device, enqueued on `stream` (default: torch's current
    stream).  Asynchronous: nothing is copied back and nothing synchronises, so the results are valid once the stream has passed the call.
    The tables come from `betas` (one beta per sweep) and `ladder` (R multipliers), built on the host and uploaded on the stream, or from
    `tables` = (T, X), int32 tensors on the device as device_tables returns them -- or the caller's own: T [n_sweeps][R][table_len <= 512]
    with no entry above 2^24 (read as uint32), X [n_events][R - 1][swap_len <= 4096]; neither is checked on the device path.  `seeds` is
    an int32 tensor [n_chains] on the device (the uint32 seeds bit for bit) or a NumPy array / list; `rungs` (optional) a uint8 tensor
    [n_chains] on the device or a NumPy array / list, a permutation of 0 .. R - 1 per ladder, which the device path cannot check either;
    `out` may be `states` itself (in place).
    Returns a dict of tensors: `state`, `energy_in`, `energy_out`, `best_energy` int32[n_chains], `best_sweep`, `n_changed`,
    `n_exchanges` int64[n_chains], `rung_out` uint8[n_chains], `pair_accepted` int64[n_chains / R][R - 1], `best_state` unless
    best_state=False, and with trace=True `energy_hist` int32 and `rung_hist` uint8 [n_chains][n_sweeps + 1].  `form` is one of FORMS:
    "counters" runs mcq_temper_counters_device (N <= 16; the same results bit for bit); an unknown form, or "counters" with a larger N,
    is a ValueError before anything else is looked at."""
    _check_form(form, N)
    n = _device_states("temper_device", N, states)
    K = int(exchange_every)
    run = _lib.temper_counters_device if form == "counters" else _lib.temper_device
    return _device_call(n, lambda n_sweeps, R, D, DX: _block(N, n, n_sweeps, first_sweep, R, K, D, DX), run, abi.TEMPER_DTYPES, states,
                        seeds, betas, ladder, K, first_sweep, rungs, tables, out, trace, best_state, stream)


def temper_queens_device(N, states, seeds, betas=None, ladder=None, Q=None, exchange_every=1, first_sweep=0, rungs=None, tables=None, out=None,
                         trace=False, best_state=True, stream=None):
    """mcq_temper3d_device on a torch uint8 tensor [n_chains][3 Q] or [n_chains][Q][3] of the current device (the final_state layout of a
    full_3d run; Q=None means N^2), enqueued on `stream` (default: torch's current stream).  Asynchronous: nothing is copied back and
    nothing synchronises.  `seeds`, `betas` and `ladder` or `tables`, `rungs` and `out` are those of temper_device, with the same checks;
    no entry of a caller's own T may exceed 2^24 (a lane of the kernel sums up to 255 entries in 32 bits), which is NOT checked here.
    Returns a dict of tensors: those of temper_device, `state` and `best_state` like `states`, and `flags` int32[n_chains] (bit 0,
    abi.HEATBATH3D_REPEATED: the slot holds two queens in one cell; bit 1, abi.TEMPER3D_HELD: a slot of its ladder does, and the whole
    ladder was handed back unmoved).  ValueError before any launch for a ladder that does not fit the LDS of a workgroup
    (abi.temper3d_lds_bytes); the message names N, R, Q and the bytes."""
    n, Qn = _device_queens("temper_queens_device", N, states, Q)
    K = int(exchange_every)
    return _device_call(n, lambda n_sweeps, R, D, DX: _block3d(N, Qn, n, n_sweeps, first_sweep, R, K, D, DX), _lib.temper3d_device, abi.TEMPER3D_DTYPES,
                        states, seeds, betas, ladder, K, first_sweep, rungs, tables, out, trace, best_state, stream)


def temper_states(N, states, seeds, betas, ladder, exchange_every=1, first_sweep=0, rungs=None, trace=False, form="lines"):
    """Tempered heat-bath sweeps of board placements on the GPU: `states` is uint8[n_chains][N*N], bytes >= N are clamped to N - 1;
    `seeds` one uint32 per chain; `betas` one beta >= 0 per sweep (len(betas) sweeps with the global indices first_sweep, ...); `ladder`
    R = 2, 4, 8 or 16 finite, positive, non-decreasing multipliers: chains [g R, (g + 1) R) form ladder g, and a slot on rung t runs
    sweep s at beta_s ladder[t].  After every sweep whose global index g has (g + 1) % exchange_every == 0 neighbouring rungs are
    offered a swap.  `rungs` (optional) is every slot's starting rung, a permutation of 0 .. R - 1 per ladder (default: slot r on rung
    r % R) -- with first_sweep and the placements what a later call carries over.
    Returns a dict of NumPy arrays with the keys of FIELDS -- those of heatbath_states, `rung_out` uint8[n_chains], `n_exchanges`
    int64[n_chains], `pair_accepted` int64[n_chains / R][R - 1] -- and with trace=True `energy_hist` and `rung_hist`
    [n_chains][len(betas) + 1].  ValueError for what the library refuses and for a ladder or a beta abi.temper_tables refuses.
    `form` is temper_device's: "lines" or "counters" (N <= 16), the same results."""
    _check_form(form, N)
    import torch

    s = _host_states(N, states)
    T, X = abi.temper_tables(betas, ladder, exchange_every, first_sweep)
    if rungs is not None:
        rungs = _host_rungs(rungs, s.shape[0])
        R = T.shape[1]
        if s.shape[0] % R == 0 and not (np.sort(rungs.reshape(-1, R), axis=1) == np.arange(R)).all():
            raise ValueError(f"rungs: every ladder must hold a permutation of 0 .. {R - 1}")
    if s.shape[0] == 0:
        _lib.temper_host(_block(N, 0, 0, first_sweep, T.shape[1], exchange_every, 1, 1))  # raises the library's refusal
    dev = torch.device("cuda", torch.cuda.current_device())
    res = temper_device(N, torch.from_numpy(s).to(dev), seeds, betas, ladder, exchange_every, first_sweep, rungs=rungs, trace=trace, form=form)
    torch.cuda.current_stream(dev).synchronize()
    return to_numpy(res)


def temper_queens(N, states, seeds, betas, ladder, Q=None, exchange_every=1, first_sweep=0, rungs=None, trace=False):
    """Tempered heat-bath queen sweeps of full_3d placements on the GPU: `states` is uint8[n_chains][3 Q] or [n_chains][Q][3] (Q triples
    (i, j, k); Q=None means N^2), bytes >= N are clamped to N - 1; `seeds`, `betas`, `ladder`, `exchange_every`, `first_sweep` and
    `rungs` are those of temper_states.  Returns a dict of NumPy arrays with the keys of FIELDS_3D -- those of temper_states, `state`
    and `best_state` uint8 shaped like the input, and `flags` (temper_queens_device) -- and with trace=True `energy_hist` and `rung_hist`
    [n_chains][len(betas) + 1].  ValueError for what the library refuses (N outside 2 .. 32, Q outside 2 .. N^3 - 1, a ladder beyond the
    LDS of a workgroup, ...) and for a ladder or a beta abi.temper_tables refuses."""
    import torch

    s = _host_queens(N, states, Q)
    T, X = abi.temper_tables(betas, ladder, exchange_every, first_sweep)
    R = T.shape[1]
    if rungs is not None:
        rungs = _host_rungs(rungs, s.shape[0])
        if s.shape[0] % R == 0 and not (np.sort(rungs.reshape(-1, R), axis=1) == np.arange(R)).all():
            raise ValueError(f"rungs: every ladder must hold a permutation of 0 .. {R - 1}")
    if s.shape[0] == 0:
        _lib.temper3d_host(_block3d(N, _queens_of(N, Q), 0, 0, first_sweep, R, exchange_every, 1, 1))  # raises the library's refusal
    dev = torch.device("cuda", torch.cuda.current_device())
    res = temper_queens_device(N, torch.from_numpy(s).to(dev), seeds, betas, ladder, Q=Q, exchange_every=exchange_every, first_sweep=first_sweep,
                               rungs=rungs, trace=trace)
    torch.cuda.current_stream(dev).synchronize()
    return to_numpy(res)


def ladder_statistics(res, n_events):
    """What a caller tunes a ladder with, from a result dict: `pair_rate` float64[R - 1], the accepted share of the offers made to
    each pair of rungs over all ladders (pair t is offered at the events of its parity), and `exchanges_per_slot`, the mean."""
    acc = np.asarray(res["pair_accepted"], dtype=np.int64)
    ladders, pairs = acc.shape
    ev = np.asarray(n_events, dtype=np.int64).reshape(-1)  # offers per parity: (even events, odd events)
    offers = np.array([ev[t & 1] for t in range(pairs)], dtype=np.float64) * ladders
    with np.errstate(divide="ignore", invalid="ignore"):
        rate = np.where(offers > 0, acc.sum(axis=0) / offers, 0.0)
    return {"pair_rate": rate, "exchanges_per_slot": float(np.asarray(res["n_exchanges"]).mean())}


def anneal_tempered(N, n_sweeps, init, schedule_params, seeds, ladder, exchange_every=1, quench=False, trace=False, mcmc_type="board", Q=None,
                    form="lines"):
    """Every ladder of `seeds` for n_sweeps tempered heat-bath sweeps under one beta schedule, beta of sweep s =
    abi.beta_values(schedule_params, n_sweeps)[s] times the multiplier of the slot's rung: ONE launch.  `init` is an init mode of the
    reference ("random", "latin", "klarner": the start placements anneal_heatbath makes) or a uint8 array [n_chains][N*N].
    Returns per chain final_state / final_energy, initial_energy, best_state / best_energy / best_sweep, n_changed, the ladder's
    figures -- final_rung, n_exchanges, pair_accepted, and ladder_statistics' pair_rate and exchanges_per_slot --, with trace=True
    energy_hist and rung_hist, and with quench=True quenched_state, quenched_energy, quench_moves (best_state through
    quench.quench_device on the same stream; quench="pairs", boards up to N = 32, takes quench.quench_pairs_device instead and adds
    quench_pair_moves, quench_rounds, quench_certified, quench_energy_single).  ValueError before anything is launched for what
    temper_states refuses.

    mcmc_type="full_3d" (default "board": everything above) runs tempered heat-bath QUEEN sweeps of Q queens in the cube (Q=None: N^2)
    through temper_queens_device: the placements are uint8[n_chains][3 Q], the start placements those of
    start_chains(..., mcmc_type="full_3d") or given ones, as anneal_heatbath makes them, the result also holds `flags`, and quench=True
    goes through quench.quench_queens_device.

    form (one of FORMS, default "lines") is the kernel the board launch runs through (temper_device's `form`; the results do not depend
    on it); "counters" needs N <= 16, and full_3d placements have the one form "lines".  An unknown form or one the placements do not
    have is a ValueError before anything else is looked at."""
    _check_form(form, N, mcmc_type)
    import torch

    from . import quench as _quench

    _quench.check_mode(quench, N, board=mcmc_type != "full_3d")
    n_sweeps = int(n_sweeps)
    if n_sweeps < 0:
        raise ValueError(f"n_sweeps must be >= 0, got {n_sweeps}")
    if isinstance(schedule_params, (list, tuple)):
        raise ValueError("anneal_tempered runs one schedule")
    seeds = _host_seeds(seeds, len(np.asarray(seeds).reshape(-1)))
    n = len(seeds)
    l = abi.temper_ladder(ladder)
    R, K = len(l), int(exchange_every)
    beta = abi.beta_values(schedule_params, n_sweeps)
    T, X = abi.temper_tables(beta, l, K, 0)
    if mcmc_type not in ("board", "full_3d"):
        raise ValueError(f"Unknown mcmc_type {mcmc_type}")
    cube = mcmc_type == "full_3d"
    max_n = abi.MAX_N_QUENCH3D if cube else abi.MAX_N_BOARD
    if not (abi.MIN_N <= int(N) <= max_n):
        raise ValueError(f"N out of range [{abi.MIN_N}, {max_n}]: {N}")
    if not cube and Q is not None:
        raise ValueError("Q is the number of queens of a full_3d placement; a board has one height per column")
    Qn = _queens_of(N, Q)
    if cube and not 2 <= Qn <= int(N) ** 3 - 1:
        raise ValueError(f"n_queens out of range [2, N^3 - 1 = {int(N) ** 3 - 1}] (0 = N^2): {Qn}")
    width = 3 * Qn if cube else int(N) * int(N)  # bytes of one placement
    if n == 0 or n % R:
        raise ValueError(f"replicas ({R}) must divide the number of chains ({n})")
    if isinstance(init, str):
        from . import experiments as _ex

        if init not in abi.INIT:
            raise ValueError(f"Unknown init_mode {init}")
        first, _ = _ex.start_chains(N, 0, init, schedule_params, seeds, mcmc_type=mcmc_type, trace=False, states=True, Q=Qn if cube else None)
        start = np.ascontiguousarray(first["final_state"], dtype=np.uint8).reshape(n, -1)
    else:
        start = _host_queens(N, init, Qn) if cube else _host_states(N, init)
    if start.shape != (n, width):
        raise ValueError(f"init must be uint8[{n}][{width}] (one placement per seed), got {start.shape}")
    dev = torch.device("cuda", torch.cuda.current_device())
    st = torch.cuda.current_stream(dev)
    quenched = None
    with torch.cuda.device(dev), torch.cuda.stream(st):
        state = torch.from_numpy(start).to(dev)
        tables = _upload_tables(T, X, dev)
        if cube:
            seg = temper_queens_device(N, state, seeds, beta, tables=tables, Q=Qn, exchange_every=K, out=state, trace=trace, stream=st)
        else:
            seg = temper_device(N, state, seeds, beta, tables=tables, exchange_every=K, out=state, trace=trace, stream=st, form=form)
        if quench:
            if cube:
                quenched = _quench.quench_queens_device(N, seg["best_state"], Q=Qn, conflicts=False, stream=st)
            else:
                quenched = _quench.hook_device(N, seg["best_state"], quench, st)
        st.synchronize()
    got = to_numpy(seg)
    res = {"initial_energy": got["energy_in"], "final_energy": got["energy_out"], "final_state": got["state"], "best_energy": got["best_energy"],
           "best_sweep": got["best_sweep"], "best_state": got["best_state"], "n_changed": got["n_changed"], "final_rung": got["rung_out"],
           "n_exchanges": got["n_exchanges"], "pair_accepted": got["pair_accepted"]}
    if cube:
        res["flags"] = got["flags"]
    events = n_sweeps // K
    res.update(ladder_statistics(got, ((events + 1) // 2, events // 2)))
    if trace:
        res["energy_hist"], res["rung_hist"] = got["energy_hist"], got["rung_hist"]
    if quenched is not None:
        _quench.hook_results(res, quenched)
    return res
