"""Heat-bath column sweeps of board placements (include/mcq.h: mcq_heatbath, where the rule is stated; csrc/mcq_heatbath.hip).

NOT a mode of the reference -- its only move is one random column, one random height and one Metropolis test --, never a default, and
labelled as such like Philox, replica exchange, population annealing and the quench.  A sweep visits every column in row-major order
and draws its new height from the Boltzmann weights of all N heights at once, so nothing is rejected.  The rule is integer-exact, so
the library's host code, the kernel and a NumPy restatement (tests/heatbath_util.py) agree bit for bit.  Boards: N = 2 .. 128
(heatbath_states*, heatbath_device).

full_3d placements have a rule and a kernel of their own (include/mcq.h: mcq_heatbath3d; csrc/mcq_heatbath3d.hip), N = 2 .. 32 and
2 <= Q <= N^3 - 1: heatbath_queens, heatbath_queens_device, heatbath_queens_host.  A sweep visits every queen in index order and draws
its new cell from the Boltzmann weights of all N^3 - Q + 1 cells that hold no other queen.  The same labels apply: NOT a mode of the
reference, never a default.  anneal_heatbath runs either under a schedule (mcmc_type="board" or "full_3d").
"""
import numpy as np

from . import _lib, abi
from .quench import _device_out, _device_queens, _device_states, _host_outputs, _host_queens, _host_states, _queens_of

FIELDS = ("state", "energy_in", "energy_out", "best_energy", "best_sweep", "best_state", "n_changed")
FIELDS_3D = FIELDS + ("flags",)
# the two kernels of the board sweep: "lines" (mcq_heatbath_device, every N, the default) tests the cells of a column's four lines;
# "counters" (mcq_heatbath_counters_device, N <= abi.MAX_N_HEATBATH_COUNTERS) reads per-line queen counters.  Same rule, same results.
FORMS = ("lines", "counters")


def _check_form(form, N):
    """ValueError for an unknown form and for the counter form beyond its largest N; nothing here touches the GPU."""
    if form not in FORMS:
        raise ValueError(f"Unknown form {form!r}: the heat-bath sweep of boards has the forms {FORMS}")
    if form == "counters" and int(N) > abi.MAX_N_HEATBATH_COUNTERS:
        raise ValueError(f'form="counters" runs N <= {abi.MAX_N_HEATBATH_COUNTERS}, got N = {int(N)}; form="lines" runs every N')


def _block(N, n, n_sweeps, first_sweep, table):
    q = abi.Heatbath()
    q.N, q.mode, q.n_chains, q.n_sweeps, q.first_sweep = int(N), abi.MODE_BOARD, int(n), int(n_sweeps), int(first_sweep)
    q.table_len = int(table.shape[1])
    return q


def _host_seeds(seeds, n):
    s = np.asarray(seeds)
    if s.size and (s.min() < 0 or s.max() > 2**32 - 1):
        raise ValueError("Seed must be between 0 and 2**32 - 1")
    s = np.ascontiguousarray(s, dtype=np.uint32).reshape(-1)
    if len(s) != n:
        raise ValueError(f"seeds must have one entry per chain: {len(s)} seeds, {n} chains")
    return s


def _host_sweeps(block, run, s, seeds, betas, dtypes, trace):
    """What the two *_host wrappers share: the seeds and the table checked, the parameter block from block(n_chains, n_sweeps, table),
    _host_outputs with best_state next to state and the trace when asked for, and the call `run` of the library."""
    n = s.shape[0]
    seeds = _host_seeds(seeds, n)
    table = abi.heatbath_table(betas)
    n_sweeps = int(np.asarray(betas).size)
    q = block(n, n_sweeps, table)
    out = _host_outputs(q, s, dtypes, like=("best_state",))
    q.seeds, q.table = seeds.ctypes.data, table.ctypes.data
    if trace:
        out["energy_hist"] = np.zeros((n, n_sweeps + 1), dtype=np.int32)
        q.energy_hist, q.hist_stride = out["energy_hist"].ctypes.data, n_sweeps + 1
    run(q)
    return out


def heatbath_states_host(N, states, seeds, betas, first_sweep=0, trace=False):
    """mcq_heatbath_host: the rule in the library's plain host code, NumPy in and out, no GPU.  Same result as heatbath_states."""
    return _host_sweeps(lambda n, n_sweeps, table: _block(N, n, n_sweeps, first_sweep, table), _lib.heatbath_host,
                        _host_states(N, states), seeds, betas, abi.HEATBATH_DTYPES, trace)


def _upload(a, dev):
    """A NumPy array to the device on torch's current stream without blocking the host: through a pinned copy."""
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).pin_memory().to(dev, non_blocking=True)


def device_table(betas, device):
    """abi.heatbath_table(betas) on the device as an int32 tensor [n_sweeps][table_len] (the uint32 weights bit for bit), uploaded on
    torch's current stream: what heatbath_device takes in place of `betas`, whole or as a slice of rows (a slice of a longer run's table
    is as good as the slice's own: a row is zero from its first zero on, so a larger table_len reads the same weights).  A caller may
    pass a tensor of its own weights in that place; every entry must then be at most 2^abi.HEATBATH_WEIGHT_BITS = 2^24 as uint32
    (include/mcq.h, item 3 of either rule), which nothing on the device path checks."""
    return _upload(abi.heatbath_table(betas).view(np.int32), device)


def _device_buffers(states, seeds, betas, out, dtypes, trace, best_state):
    """What heatbath_device and heatbath_queens_device share, on torch's current stream and device: the table and the seeds on the device
    (checked when given as tensors, uploaded otherwise) and the dict of result tensors.  Returns (table, n_sweeps, seeds, results)."""
    import torch

    dev, n = states.device, int(states.shape[0])
    if isinstance(betas, torch.Tensor):  # the rows of device_table, already on the device
        tab = betas
        if tab.dtype != torch.int32 or tab.device != dev or tab.dim() != 2 or not tab.is_contiguous() or not 1 <= tab.shape[1] <= abi.MAX_HEATBATH_TABLE:
            raise ValueError("a table on the device is a contiguous int32 tensor [n_sweeps][table_len <= 512] (device_table)")
        n_sweeps = int(tab.shape[0])
    else:
        n_sweeps = int(np.asarray(betas).size)
        tab = device_table(betas, dev)
    if isinstance(seeds, torch.Tensor):
        if seeds.dtype != torch.int32 or seeds.device != dev or not seeds.is_contiguous() or tuple(seeds.shape) != (n,):
            raise ValueError("seeds must be a contiguous int32 tensor [n_chains] on the device of states (the uint32 seeds bit for bit)")
    else:
        seeds = _upload(_host_seeds(seeds, n).view(np.int32), dev)
    res = {"state": _device_out(out, states)}
    tdt = {np.int32: torch.int32, np.int64: torch.int64}
    for k, dt in dtypes.items():
        res[k] = torch.empty(n, dtype=tdt[dt], device=dev)
    if best_state:
        res["best_state"] = torch.empty_like(states)
    if trace:
        res["energy_hist"] = torch.empty((n, n_sweeps + 1), dtype=torch.int32, device=dev)
    return tab, n_sweeps, seeds, res


def _point(q, states, seeds, tab, res, dtypes, n_sweeps):
    """The device pointers of a call into its parameter block."""
    q.seeds, q.table, q.state_in, q.state_out = seeds.data_ptr(), tab.data_ptr(), states.data_ptr(), res["state"].data_ptr()
    for k in tuple(dtypes) + ("best_state", "energy_hist"):
        if k in res:
            setattr(q, k, res[k].data_ptr())
    q.hist_stride = n_sweeps + 1


def heatbath_device(N, states, seeds, betas, first_sweep=0, out=None, trace=False, best_state=True, stream=None, form="lines"):
    """mcq_heatbath_device on a torch uint8 tensor [n_chains][N*N] of the current device, enqueued on `stream` (default: torch's current
    stream).  Asynchronous: nothing is copied back and nothing synchronises, so the results are valid once the stream has passed the
    call.  `seeds` is an int32 tensor [n_chains] on the device holding the uint32 seeds bit for bit (or a NumPy array / list, which is
    uploaded on the stream); `betas` holds one beta per sweep (NumPy / list: the weight table is built on the host and uploaded on the
    stream through a pinned copy) or is device_table's tensor, or a slice of its rows.  `out` (optional) is the tensor the placements go to; it may be `states` itself (in place), default a new one.
    Returns a dict of tensors: `state`, `energy_in` (the recount of the input), `energy_out`, `best_energy` int32[n_chains],
    `best_sweep`, `n_changed` int64[n_chains], `best_state` unless best_state=False, and with trace=True `energy_hist`
    int32[n_chains][n_sweeps + 1].  `form` is one of FORMS: "counters" runs mcq_heatbath_counters_device (N <= 16; the same results bit
    for bit); an unknown form, or "counters" with a larger N, is a ValueError before anything else is looked at.
    A `betas` tensor of the caller's own weights must hold no entry above 2^24 (read as uint32): beyond it the kernels' 32-bit sums can
    wrap (W < 2^32 at N = 128 needs it).  It is NOT checked here: a check would read the tensor back and synchronise."""
    _check_form(form, N)
    import torch

    n = _device_states("heatbath_device", N, states)
    dev = states.device
    st = torch.cuda.current_stream(dev) if stream is None else stream
    with torch.cuda.device(dev), torch.cuda.stream(st):
        tab, n_sweeps, seeds, res = _device_buffers(states, seeds, betas, out, abi.HEATBATH_DTYPES, trace, best_state)
        q = _block(N, n, n_sweeps, first_sweep, tab)
        _point(q, states, seeds, tab, res, abi.HEATBATH_DTYPES, n_sweeps)
        (_lib.heatbath_counters_device if form == "counters" else _lib.heatbath_device)(q, st)
        seeds.record_stream(st), tab.record_stream(st)  # (the kernel reads them after this call has returned)
    return res


def to_numpy(res):
    """The dict heatbath_device returned, as NumPy arrays.  The stream must have passed the call."""
    return {k: t.cpu().numpy() for k, t in res.items()}


def heatbath_states(N, states, seeds, betas, first_sweep=0, trace=False, form="lines"):
    """Heat-bath sweeps of board placements on the GPU: `states` is uint8[n_chains][N*N] (the final_state / best_state layout; one board
    of N*N heights is taken as one chain), bytes >= N are clamped to N - 1; `seeds` one uint32 per chain; `betas` one beta >= 0 per
    sweep (len(betas) sweeps are run, with the global indices first_sweep, first_sweep + 1, ...).  Returns a dict of NumPy arrays:
    `state` (the placements after the sweeps), `energy_in` (the energy of the input, recounted on the device), `energy_out`,
    `best_energy`, `best_sweep` (sweeps of this call after which best_energy was first reached; 0 = the input), `best_state`,
    `n_changed` (updates that changed a height, of len(betas) N^2) and with trace=True `energy_hist` int32[n_chains][len(betas) + 1].
    ValueError for what the library refuses (N outside 2 .. 128, no chain, a negative first_sweep, ...) and for a negative beta.
    `form` is heatbath_device's: "lines" or "counters" (N <= 16), the same results."""
    _check_form(form, N)
    import torch

    s = _host_states(N, states)
    if s.shape[0] == 0:
        abi.heatbath_table(betas)
        _lib.heatbath_host(_block(N, 0, 0, first_sweep, abi.heatbath_table([])))  # raises the library's refusal
    dev = torch.device("cuda", torch.cuda.current_device())
    res = heatbath_device(N, torch.from_numpy(s).to(dev), seeds, betas, first_sweep=first_sweep, trace=trace, form=form)
    torch.cuda.current_stream(dev).synchronize()
    return to_numpy(res)


def _block3d(N, Q, n, n_sweeps, first_sweep, table):
    q = abi.Heatbath3D()
    q.N, q.n_queens, q.n_chains, q.n_sweeps, q.first_sweep = int(N), int(Q), int(n), int(n_sweeps), int(first_sweep)
    q.table_len = int(table.shape[1])
    return q


def heatbath_queens_host(N, states, seeds, betas, Q=None, first_sweep=0, trace=False):
    """mcq_heatbath3d_host: the full_3d rule in the library's plain host code, NumPy in and out, no GPU.  Same result as heatbath_queens."""
    return _host_sweeps(lambda n, n_sweeps, table: _block3d(N, _queens_of(N, Q), n, n_sweeps, first_sweep, table), _lib.heatbath3d_host,
                        _host_queens(N, states, Q), seeds, betas, abi.HEATBATH3D_DTYPES, trace)


def heatbath_queens_device(N, states, seeds, betas, Q=None, first_sweep=0, out=None, trace=False, best_state=True, stream=None):
    """mcq_heatbath3d_device on a torch uint8 tensor [n_chains][3 Q] or [n_chains][Q][3] of the current device (the final_state layout of
    a full_3d run; Q=None means N^2), enqueued on `stream` (default: torch's current stream).  Asynchronous: nothing is copied back and
    nothing synchronises.  `seeds`, `betas` and `out` are those of heatbath_device: tensors already on the device or host values that are
    uploaded on the stream; `out` may be `states` itself (in place).  Returns a dict of tensors: `state` like `states`, `energy_in`,
    `energy_out`, `best_energy`, `flags` int32[n_chains], `best_sweep`, `n_changed` int64[n_chains], `best_state` unless
    best_state=False, and with trace=True `energy_hist` int32[n_chains][n_sweeps + 1].
    A `betas` tensor of the caller's own weights must hold no entry above 2^24 (read as uint32): a lane of the kernel sums up to 34
    entries in 32 bits.  It is NOT checked here: a check would read the tensor back and synchronise."""
    import torch

    n, Qn = _device_queens("heatbath_queens_device", N, states, Q)
    dev = states.device
    st = torch.cuda.current_stream(dev) if stream is None else stream
    with torch.cuda.device(dev), torch.cuda.stream(st):
        tab, n_sweeps, seeds, res = _device_buffers(states, seeds, betas, out, abi.HEATBATH3D_DTYPES, trace, best_state)
        q = _block3d(N, Qn, n, n_sweeps, first_sweep, tab)
        _point(q, states, seeds, tab, res, abi.HEATBATH3D_DTYPES, n_sweeps)
        _lib.heatbath3d_device(q, st)
        seeds.record_stream(st), tab.record_stream(st)  # (the kernel reads them after this call has returned)
    return res


def heatbath_queens(N, states, seeds, betas, Q=None, first_sweep=0, trace=False):
    """Heat-bath sweeps of full_3d placements on the GPU: `states` is uint8[n_chains][3 Q] or [n_chains][Q][3] (Q triples (i, j, k);
    Q=None means N^2), bytes >= N are clamped to N - 1; `seeds` one uint32 per chain; `betas` one beta >= 0 per sweep.  Returns a dict of
    NumPy arrays with the keys of FIELDS_3D: `state` uint8[n_chains][3 Q], `energy_in` (the energy of the input, recounted on the
    device), `energy_out`, `best_energy`, `best_sweep`, `best_state`, `n_changed` (updates that changed a cell, of len(betas) Q) and
    `flags` (bit 0, abi.HEATBATH3D_REPEATED: an input with two queens in one cell, which is recounted and handed back unmoved), and with
    trace=True `energy_hist` int32[n_chains][len(betas) + 1].  ValueError for what the library refuses (N outside 2 .. 32, Q outside
    2 .. N^3 - 1, no chain, a negative first_sweep, ...) and for a negative beta."""
    import torch

    s = _host_queens(N, states, Q)
    if s.shape[0] == 0:
        abi.heatbath_table(betas)
        _lib.heatbath3d_host(_block3d(N, _queens_of(N, Q), 0, 0, first_sweep, abi.heatbath_table([])))  # raises the library's refusal
    dev = torch.device("cuda", torch.cuda.current_device())
    res = heatbath_queens_device(N, torch.from_numpy(s).to(dev), seeds, betas, Q=Q, first_sweep=first_sweep, trace=trace)
    torch.cuda.current_stream(dev).synchronize()
    out = to_numpy(res)
    out["state"], out["best_state"] = out["state"].reshape(s.shape), out["best_state"].reshape(s.shape)
    return out


def check(n_chains, n_sweeps, resample_every, population=None):
    """What anneal_heatbath does not resample, as ValueError before anything is launched -- population.check's refusals, for the same
    reasons, with steps read as sweeps.  Returns (S, R): the segment length in sweeps and the population size in force."""
    n, S = int(n_chains), int(resample_every)
    if S <= 0:
        raise ValueError(f"resample_every must be positive, got {resample_every}")
    if int(n_sweeps) < 1:
        raise ValueError("population annealing needs at least one sweep")
    R = n if population is None else int(population)
    if R <= 0 or R % 16 or R > abi.MAX_POPULATION:
        raise ValueError(f"a population is a positive multiple of 16 chains, at most 2^19, got {R}")
    if n % R:
        raise ValueError(f"the population ({R}) must divide the number of chains ({n})")
    return S, R


def anneal_heatbath(N, n_sweeps, init, schedule_params, seeds, resample_every=None, population=None, resample_seed=0, quench=False, trace=False,
                    mcmc_type="board", Q=None, form="lines", hops=0, hop_kick=2, tabu_iters=0, tabu_tenure=10, tabu_tenure_rand=0):
    """Every chain of `seeds` for n_sweeps heat-bath sweeps under one beta schedule, beta of sweep s = abi.beta_values(schedule_params,
    n_sweeps)[s] (the reference's schedules, evaluated per sweep instead of per step).

    `init` is an init mode of the reference ("random", "latin", "klarner": the placements are those of start_chains(N, 0, init, ...),
    the reference's own initial state of chain seeds[r]) or a uint8 array [n_chains][N*N] of placements.
    resample_every = S (None: independent chains): the chains run as segments of S sweeps and between two segments they are resampled
    inside populations of `population` consecutive chains (None: all) by mcq_resample_device, with the dbeta tables and offset words of
    population.boundaries (steps read as sweeps); everything is on one stream with one synchronise at the end.

    Returns `res`, and (res, lineage) when resampling, `lineage` being the dict anneal_population returns.  `res` holds per chain
    final_state / final_energy, initial_energy, best_state / best_energy / best_sweep (in whole-run sweeps; a later segment moves them
    only by a strictly lower energy), n_changed, `energy_hist` int32[n_chains][n_sweeps + 1] with trace=True (segments joined by dropping
    each later segment's entry 0, as anneal_population does), and with quench=True `quenched_state`, `quenched_energy`, `quench_moves`
    (best_state through quench.quench_device on the same stream).  quench="pairs" (boards up to N = 32) sends best_state through
    quench.quench_pairs_device instead, the pair-move quench: the same three fields, and `quench_pair_moves`, `quench_rounds`,
    `quench_certified`, `quench_energy_single` (what quench=True would have reached).

    mcmc_type="full_3d" (default "board": everything above) runs heat-bath QUEEN sweeps of Q queens in the cube (Q=None: N^2) through
    heatbath_queens_device: the placements are uint8[n_chains][3 Q], the start placements those of start_chains(..., mcmc_type="full_3d")
    or given ones, the segments, boundaries and fold are the same, `res` also holds `flags` (of the last segment), and quench=True goes
    through quench.quench_queens_device.

    hops = K > 0 (full_3d only; default 0: nothing changes) sends best_state -- the quenched one with quench=True -- through K hops of
    quench.hop_queens_device with kick = hop_kick and slack 0 on the same stream, seeded with the seeds of the run: `res` gains
    `hopped_state`, `hopped_energy` (the best of the hops: best_state and best_energy of that call), `hop_accepted`, `hop_improved` and
    `hop_best_hop`.  Boards refuse it: their hops are drivers.run_competition(hops=...).

    tabu_iters = K > 0 (full_3d only; default 0: nothing changes; refused together with hops) sends best_state -- the quenched one
    with quench=True -- through K iterations of quench.tabu_queens_device with tenure = tabu_tenure and tenure_rand = tabu_tenure_rand
    on the same stream, seeded with the seeds of the run: `res` gains `tabu_state`, `tabu_energy` (the best of the walk: best_state
    and best_energy of that call), `tabu_best_iter` and `tabu_moves`.  Boards refuse it: their walk is
    drivers.run_competition(tabu_iters=...).

    form (one of FORMS, default "lines") is the kernel every board segment runs through (heatbath_device's `form`; the results do not
    depend on it); "counters" needs N <= 16, and full_3d placements have the one form "lines".

    ValueError before anything is launched: an unknown form or one the placements do not have, a negative beta, and with resampling what anneal_population refuses for the same reasons -- a
    schedule that decreases over a segment, a resample_every <= 0, a population that does not divide the chains, is no multiple of 16 or
    exceeds 2^19."""
    if mcmc_type == "full_3d" and form != "lines":
        raise ValueError(f'the heat-bath queen sweep of full_3d placements has the one form "lines", got form={form!r}')
    _check_form(form, N)
    import ctypes as C

    import torch

    from . import population as _pop
    from . import quench as _quench

    _quench.check_mode(quench, N, board=mcmc_type != "full_3d")
    hops = int(hops)
    if hops < 0:
        raise ValueError(f"hops must be >= 0, got {hops}")
    if hops and mcmc_type != "full_3d":
        raise ValueError('hops: anneal_heatbath hops full_3d placements only (mcmc_type="full_3d"); boards hop through run_competition(hops=...)')
    if hops and not 1 <= int(hop_kick) <= abi.MAX_HOP_KICK:
        raise ValueError(f"hop_kick out of range [1, {abi.MAX_HOP_KICK}]: {hop_kick}")
    tabu_iters = int(tabu_iters)
    _quench.check_tabu_queens(tabu_iters, tabu_tenure, tabu_tenure_rand, hops, N, Q, board=mcmc_type != "full_3d")

    n_sweeps = int(n_sweeps)
    if n_sweeps < 0:
        raise ValueError(f"n_sweeps must be >= 0, got {n_sweeps}")
    if isinstance(schedule_params, (list, tuple)):
        raise ValueError("anneal_heatbath runs one schedule")
    seeds = _host_seeds(seeds, len(np.asarray(seeds).reshape(-1)))
    n = len(seeds)
    beta = abi.beta_values(schedule_params, n_sweeps)
    abi.heatbath_table(beta[:1])  # a negative beta is refused here
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
    Q = 3 * Qn if cube else int(N) * int(N)  # bytes of one placement
    if cube:  # one segment of sweeps on the device, and the quench that goes with the placements
        def sweep(*a, **kw):
            return heatbath_queens_device(*a, Q=Qn, **kw)
    else:
        def sweep(*a, **kw):
            return heatbath_device(*a, form=form, **kw)
    b = None
    if resample_every is not None:
        S, R = check(n, n_sweeps, resample_every, population)
        pops = n // R
        b = _pop.boundaries(schedule_params, n_sweeps, S, pops, resample_seed)
        lengths = b["lengths"]
    else:
        lengths = [n_sweeps]
    abi.heatbath_table(beta)
    K = len(lengths)
    if isinstance(init, str):
        from . import experiments as _ex

        if init not in abi.INIT:
            raise ValueError(f"Unknown init_mode {init}")
        first, _ = _ex.start_chains(N, 0, init, schedule_params, seeds, mcmc_type=mcmc_type, trace=False, states=True, Q=Qn if cube else None)
        start = np.ascontiguousarray(first["final_state"], dtype=np.uint8).reshape(n, -1)
    else:
        start = _host_queens(N, init, Qn) if cube else _host_states(N, init)
    if start.shape != (n, Q):
        raise ValueError(f"init must be uint8[{n}][{Q}] (one placement per seed), got {start.shape}")

    dev = torch.device("cuda", torch.cuda.current_device())
    st = torch.cuda.current_stream(dev)
    with torch.cuda.device(dev), torch.cuda.stream(st):
        i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)  # noqa: E731
        i64 = lambda *shape: torch.empty(shape, dtype=torch.int64, device=dev)  # noqa: E731
        state = torch.from_numpy(start).to(dev)
        dseeds = torch.from_numpy(seeds.view(np.int32).copy()).to(dev)
        dtab = device_table(beta, dev)  # the whole run's rows, uploaded once; a segment reads its slice
        hist = i32(n, n_sweeps + 1) if trace else None
        quenched = hopped = walked = None
        if b is None:
            seg = sweep(N, state, dseeds, dtab if n_sweeps else [], first_sweep=0, out=state, trace=trace, stream=st)  # one call, in place
            hist = seg.get("energy_hist")
            acc = {"best_energy": seg["best_energy"], "steps_to_best": seg["best_sweep"], "n_accepted": seg["n_changed"], "best_state": seg["best_state"]}
            e0, e1 = seg["energy_in"], seg["energy_out"]
        else:
            acc = {"best_energy": i32(n), "steps_to_best": i64(n), "n_accepted": i64(n), "best_state": torch.empty((n, Q), dtype=torch.uint8, device=dev)}
            pop_state = torch.empty((n, Q), dtype=torch.uint8, device=dev)
            final = torch.empty((n, Q), dtype=torch.uint8, device=dev)
            seg_e0, seg_e1, received = i32(K, n), i32(K, n), i32(max(K - 1, 1), n)
            parents, stats = i32(max(K - 1, 1), n), i64(max(K - 1, 1), pops, 3)
            tables = torch.from_numpy(b["tables"].view(np.int32)).to(dev)
            offsets = torch.from_numpy(b["offsets"].view(np.int32).reshape(K - 1, pops).copy()).to(dev) if K > 1 else None
            probe = abi.Resample()
            probe.n_chains = n
            scratch = torch.empty(max(8, int(_lib.lib().mcq_resample_scratch_bytes(C.byref(probe)))), dtype=torch.uint8, device=dev)
            done = 0
            keep = []
            for k, L in enumerate(lengths):
                seg = sweep(N, state, dseeds, dtab[done: done + L], first_sweep=done, out=final, trace=trace, stream=st)
                keep.append(seg)
                seg_e0[k].copy_(seg["energy_in"]), seg_e1[k].copy_(seg["energy_out"])
                r = abi.Resample()
                r.n_chains, r.population, r.state_bytes, r.first_step = n, R, Q, done
                r.seg_best_energy, r.seg_steps_to_best, r.seg_n_accepted = seg["best_energy"].data_ptr(), seg["best_sweep"].data_ptr(), seg["n_changed"].data_ptr()
                r.seg_best_state = seg["best_state"].data_ptr()
                r.run_best_energy, r.run_steps_to_best, r.run_n_accepted = acc["best_energy"].data_ptr(), acc["steps_to_best"].data_ptr(), acc["n_accepted"].data_ptr()
                r.run_best_state = acc["best_state"].data_ptr()
                if k < K - 1:
                    r.table, r.table_len = tables.data_ptr() + 4 * int(b["table_off"][k]), int(b["table_len"][k])
                    r.offsets, r.energies = offsets[k].data_ptr(), seg["energy_out"].data_ptr()
                    r.state_in, r.state_out = final.data_ptr(), pop_state.data_ptr()
                    r.parent, r.stats, r.energy_out = parents[k].data_ptr(), stats[k].data_ptr(), received[k].data_ptr()
                _lib.resample_device(r, scratch, st)
                if trace:
                    if k == 0:
                        hist[:, : L + 1].copy_(seg["energy_hist"])
                    else:  # entry 0 of a later segment is the entry before, again -- of the resampled placements
                        hist[:, done + 1: done + L + 1].copy_(seg["energy_hist"][:, 1:])
                state = pop_state
                done += L
            state = final
            e0, e1 = seg_e0[0], seg_e1[K - 1]
        if quench:  # behind the last fold, which has written acc["best_state"]; same stream, nothing waited for
            if cube:
                quenched = _quench.quench_queens_device(N, acc["best_state"], Q=Qn, conflicts=False, stream=st)
            else:
                quenched = _quench.hook_device(N, acc["best_state"], quench, st)
        if hops:  # behind the quench when there is one, whose placements it takes; same stream, nothing waited for
            hopped = _quench.hop_queens_device(N, quenched["state"] if quenched is not None else acc["best_state"], dseeds, hops, Q=Qn,
                                               kick=int(hop_kick), stream=st)
        if tabu_iters:  # in the place of the hops: behind the quench when there is one; same stream, nothing waited for
            walked = _quench.tabu_queens_device(N, quenched["state"] if quenched is not None else acc["best_state"], dseeds, tabu_iters, Q=Qn,
                                                tenure=int(tabu_tenure), tenure_rand=int(tabu_tenure_rand), stream=st)
        st.synchronize()

    res = {"initial_energy": e0.cpu().numpy(), "final_energy": e1.cpu().numpy(), "final_state": state.cpu().numpy(),
           "best_energy": acc["best_energy"].cpu().numpy(), "best_sweep": acc["steps_to_best"].cpu().numpy(),
           "best_state": acc["best_state"].cpu().numpy(), "n_changed": acc["n_accepted"].cpu().numpy()}
    if cube:
        res["flags"] = seg["flags"].cpu().numpy()
    if trace:
        res["energy_hist"] = hist.cpu().numpy()
    if quenched is not None:
        _quench.hook_results(res, quenched)
    if hopped is not None:
        res["hopped_state"], res["hopped_energy"] = hopped["best_state"].cpu().numpy(), hopped["best_energy"].cpu().numpy()
        res["hop_accepted"], res["hop_improved"] = hopped["n_accepted"].cpu().numpy(), hopped["n_improved"].cpu().numpy()
        res["hop_best_hop"] = hopped["best_hop"].cpu().numpy()
    if walked is not None:
        res["tabu_state"], res["tabu_energy"] = walked["best_state"].cpu().numpy(), walked["best_energy"].cpu().numpy()
        res["tabu_best_iter"], res["tabu_moves"] = walked["best_iter"].cpu().numpy(), walked["n_moves"].cpu().numpy()
    if b is None:
        return res
    par = parents[: K - 1].cpu().numpy()
    sts = stats[: K - 1].cpu().numpy()
    lineage = {"parents": par, "distinct_parents": sts[:, :, 0].copy(), "weight_sum": sts[:, :, 1].copy(), "e_min": sts[:, :, 2].copy(),
               "ancestors": _pop.ancestors_of(par, n), "segment_initial_energy": seg_e0.cpu().numpy(), "segment_final_energy": seg_e1.cpu().numpy(),
               "received_energy": received[: K - 1].cpu().numpy(), "lengths": list(lengths), "population": R, "dbeta": b["dbeta"]}
    return res, lineage
