"""The n-fold way of Bortz, Kalos and Lebowitz for board placements (include/mcq.h: mcq_nfold, where the rule is stated;
csrc/mcq_nfold.hip).

NOT a mode of the reference -- its sampler proposes one random column and one random height per step and rejects most of them --,
never a default, and labelled as such like Philox, the heat baths and the searches.  A chain holds the acceptance weight of all
N^2 (N - 1) moves of its board, draws the next accepted move in proportion to its weight and advances the clock by the time the
Metropolis chain would have spent rejecting: the reference's Metropolis dynamics, the same stationary distribution and the same time
axis in Metropolis steps, at a cost per EVENT that does not grow as the acceptance rate falls.  The rule is integer-exact, so the
library's host code, the kernel and a NumPy restatement (tests/nfold_util.py) agree bit for bit.  Boards, N = 2 .. 32.

full_3d placements have a rule and a kernel of their own (include/mcq.h: mcq_nfold3d; csrc/mcq_nfold3d.hip), N = 2 .. 32 and
2 <= Q <= N^3 - 1: nfold_queens, nfold_queens_device, nfold_queens_host.  A step of the reference there proposes one of
Q (N^3 - Q) moves, a queen to a cell that holds no queen; the chain draws among all of them by their acceptance weights.  The same
labels apply, and tests/nfold3d_util.py restates the rule.

A call runs segments of seg_steps Metropolis steps, beta constant inside each: weight_tables gives the rows, clock_tables the clock
("exp": exponential waiting times, the Metropolis chain's own; "mean": their expectation).  nfold_states_host, nfold_device and
nfold_states run them; anneal_nfold runs a whole schedule.  A run cut at a segment boundary is the unbroken run when `state`,
`need_out` -> need_in, `events_out` -> events_in and first_seg are carried over.
"""
import numpy as np

from . import _lib, abi
from .quench import (_Search, _device_call, _device_queens, _device_states, _hop_seeds, _host_call, _host_queens, _host_states, _queens_of,
                     _round_trip)

FIELDS = ("state", "best_state", "energy_in", "energy_out", "best_energy", "best_step", "events_out", "n_uphill", "n_flat", "need_out", "weight_out",
          "energy_hist")
CLOCKS = ("exp", "mean")


def weight_tables(betas, max_len=abi.MAX_NFOLD_TABLE):
    """The weight rows of an n-fold call (include/mcq.h, n-fold rule, item 2): T[s][d] = floor(2^24 exp(-beta_s d)) as uint32 for
    d = 0 .. D - 1, one row per segment; D = 1 + the first d with T = 0 over the rows, at most max_len (128, the boards' bound;
    abi.MAX_NFOLD3D_TABLE = 512 for full_3d placements), the rows zero-padded.  NumPy's exp / floor on float64, as abi.heatbath_table
    builds its rows.  No beta gives uint32[0][1]."""
    b = np.ascontiguousarray(betas, dtype=np.float64).reshape(-1)
    if not (np.isfinite(b).all() and (b >= 0.0).all()):
        raise ValueError("the n-fold way needs finite beta >= 0 for every segment")
    if b.size == 0:
        return np.zeros((0, 1), dtype=np.uint32)
    d = np.arange(int(max_len), dtype=np.float64)
    t = np.floor(float(1 << abi.NFOLD_WEIGHT_BITS) * np.exp(-b[:, None] * d[None, :])).astype(np.uint32)
    support = int((t != 0).any(axis=0).sum())  # the rows fall monotonically: the first all-zero d
    return np.ascontiguousarray(t[:, : min(support + 1, int(max_len))])


def clock_tables(clock="exp"):
    """(clock_ln2, clock_table uint32[256]) of an n-fold call (include/mcq.h, n-fold rule, item 5).  "exp": clock_ln2 = round(2^24 ln 2)
    and clock_table[i] = round(-2^24 ln((256 + i + 1/2) / 512)), an exponential variate of mean 1 to about 1e-6, which makes the chain
    the Metropolis chain in law; "mean": 0 and a table of 2^24, the deterministic expected waiting time.  A pair (clock_ln2, table) of
    the caller's own is handed back checked."""
    if isinstance(clock, str):
        if clock not in CLOCKS:
            raise ValueError(f"Unknown clock {clock!r}: the n-fold way has the clocks {CLOCKS}")
        if clock == "mean":
            return 0, np.full(256, 1 << 24, dtype=np.uint32)
        i = np.arange(256, dtype=np.float64)
        return int(round(float(1 << 24) * np.log(2.0))), np.round(-float(1 << 24) * np.log((256.0 + i + 0.5) / 512.0)).astype(np.uint32)
    ln2, table = clock
    table = np.ascontiguousarray(table, dtype=np.uint32).reshape(-1)
    if table.shape != (256,):
        raise ValueError(f"a clock table is uint32[256], got {table.shape}")
    return int(ln2), table


def _block(N, n, n_segs, seg_steps, first_seg, table_len, clock_ln2):
    q = abi.Nfold()
    q.N, q.mode, q.n_chains, q.n_segs, q.first_seg, q.seg_steps = int(N), abi.MODE_BOARD, int(n), int(n_segs), int(first_seg), int(seg_steps)
    q.table_len, q.clock_ln2 = int(table_len), int(clock_ln2)
    return q


_NFOLD = _Search(_block, abi.NFOLD_DTYPES, _lib.nfold_host, _lib.nfold_device, ("best_state",), True)


def _host_tables(tables):
    t = np.ascontiguousarray(tables, dtype=np.uint32)
    if t.ndim != 2 or t.shape[1] < 1:
        raise ValueError(f"tables must be uint32[n_segs][table_len] (weight_tables), got {t.shape}")
    return t


def _per_chain(name, a, n, dtype):
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype=dtype).reshape(-1)
    if a.shape[0] != n:
        raise ValueError(f"{name} must have one entry per chain: {a.shape[0]} entries, {n} chains")
    return a


def nfold_states_host(N, states, seeds, tables, seg_steps, first_seg=0, clock="exp", need_in=None, events_in=None, hist=False):
    """mcq_nfold_host: the rule in the library's plain host code, NumPy in and out, no GPU.  Same result as nfold_states."""
    s = _host_states(N, states)
    n, t = s.shape[0], _host_tables(tables)
    ln2, ct = clock_tables(clock)
    width = t.shape[0] + 1
    ins = {"table": t, "clock_table": ct, "need_in": _per_chain("need_in", need_in, n, np.uint64), "events_in": _per_chain("events_in", events_in, n, np.int64)}
    return _host_call(_NFOLD, (N,), s, (t.shape[0], seg_steps, first_seg, t.shape[1], ln2), {"energy_hist": (n, width)} if hist else {}, seeds, width,
                      inputs=lambda: {k: a for k, a in ins.items() if a is not None and a.size})


def _on_device(name, a, dev, shape, what):
    """`a` as an int32 or int64 tensor on `dev`: a tensor is checked, a NumPy array (its bits) is uploaded on torch's current stream."""
    import torch

    from .heatbath import _upload

    if a is None:
        return None
    if isinstance(a, torch.Tensor):
        ok = a.device == dev and a.is_contiguous() and a.dtype == what and (shape is None or tuple(a.shape) == shape)
        if not ok:
            raise ValueError(f"{name} on the device is a contiguous {what} tensor{'' if shape is None else ' ' + str(list(shape))} on the device of states")
        return a
    if a.size == 0:
        return torch.empty(a.shape, dtype=what, device=dev)
    return _upload(a.view(np.int32 if what == torch.int32 else np.int64), dev)


def _enqueue(d, fn, dims, n, states, seeds, tables, seg_steps, first_seg, clock, need_in, events_in, hist, out, stream):
    """What the two device wrappers share behind the check of `states`: the rows, the clock, the seeds, the need and the event counters
    brought to the device of states on `stream` (default: torch's current stream), the search `d` enqueued there through _device_call for
    the wrapper `fn`, and every input kept alive until the stream has passed the call.  Returns the dict of result tensors."""
    import torch

    dev = states.device
    st = torch.cuda.current_stream(dev) if stream is None else stream
    with torch.cuda.device(dev), torch.cuda.stream(st):
        if isinstance(tables, torch.Tensor):
            if tables.dim() != 2 or tables.shape[1] < 1:
                raise ValueError(f"tables must be [n_segs][table_len] (weight_tables), got {tuple(tables.shape)}")
            tab = _on_device("tables", tables, dev, None, torch.int32)
        else:
            tab = _on_device("tables", _host_tables(tables), dev, None, torch.int32)
        if isinstance(clock, tuple) and isinstance(clock[1], torch.Tensor):
            ln2, ct = int(clock[0]), _on_device("a clock table", clock[1], dev, (256,), torch.int32)
        else:
            ln2, ct = clock_tables(clock)
            ct = _on_device("a clock table", ct, dev, (256,), torch.int32)
        if not isinstance(seeds, torch.Tensor):
            seeds = _on_device("seeds", _hop_seeds(seeds, n), dev, (n,), torch.int32)
        need = _on_device("need_in", need_in if isinstance(need_in, torch.Tensor) else _per_chain("need_in", need_in, n, np.uint64), dev, (n,), torch.int64)
        events = _on_device("events_in", events_in if isinstance(events_in, torch.Tensor) else _per_chain("events_in", events_in, n, np.int64), dev, (n,),
                            torch.int64)
        n_segs, width = int(tab.shape[0]), int(tab.shape[0]) + 1
        ins = {"table": tab, "clock_table": ct, "need_in": need, "events_in": events}
        res = _device_call(d, fn, dims, n, states, (n_segs, seg_steps, first_seg, int(tab.shape[1]), ln2), {"energy_hist": (n, width)} if hist else {}, seeds, width,
                           inputs=lambda: {k: t for k, t in ins.items() if t is not None and t.numel()}, out=out, stream=st)
        for t in (seeds,) + tuple(t for t in ins.values() if t is not None):
            t.record_stream(st)  # (the kernel reads them after this call has returned)
    return res


def nfold_device(N, states, seeds, tables, seg_steps, first_seg=0, clock="exp", need_in=None, events_in=None, hist=False, out=None, stream=None):
    """mcq_nfold_device on a torch uint8 tensor [n_chains][N*N] of the current device, enqueued on `stream` (default: torch's current
    stream).  ONE kernel whatever the number of segments is.  Asynchronous: nothing is copied back and nothing synchronises, so the
    results are valid once the stream has passed the call.  `seeds` is an int32 or uint32 tensor [n_chains] on the device (the seeds' 32
    bits, whatever the sign) or a NumPy array / list, which is uploaded on the stream; `tables` is weight_tables' array or an int32
    tensor [n_segs][table_len] of its bits on the device, `clock` a name of CLOCKS or a pair (clock_ln2, table) whose table may be an
    int32 tensor [256] on the device; need_in (the uint64 bits as int64) and events_in are int64 tensors [n_chains] or NumPy arrays.
    The entries of tensors are NOT checked (a check would read them back): a weight is at most 2^24, a clock entry at most 2^26, a
    need below 2^45.  `out` (optional) is the tensor the placements go to; it may be `states` itself (in place), default a new one.
    Returns a dict of tensors with the fields of FIELDS: `state` and `best_state` uint8 like `states`; `energy_in`, `energy_out`,
    `best_energy` int32[n_chains]; `best_step`, `events_out`, `n_uphill`, `n_flat` int64[n_chains]; `need_out` and `weight_out`
    int64[n_chains] holding the uint64 bits; and with hist=True `energy_hist` int32[n_chains][n_segs + 1]."""
    return _enqueue(_NFOLD, "nfold_device", (N,), _device_states("nfold_device", N, states), states, seeds, tables, seg_steps, first_seg, clock, need_in,
                    events_in, hist, out, stream)


def to_numpy(res):
    """The dict nfold_device returned, as NumPy arrays (need_out and weight_out as uint64).  The stream must have passed the call."""
    out = {k: t.cpu().numpy() for k, t in res.items()}
    for k in ("need_out", "weight_out"):
        if k in out:
            out[k] = out[k].view(np.uint64)
    return out


def nfold_states(N, states, seeds, tables, seg_steps, first_seg=0, clock="exp", need_in=None, events_in=None, hist=False):
    """The n-fold way on the GPU: `states` is uint8[n_chains][N*N] (one board of N*N heights is taken as one chain), bytes >= N are
    clamped to N - 1; `seeds` is uint32[n_chains]; `tables` holds one weight row per segment (weight_tables) and every segment lasts
    seg_steps Metropolis steps; `clock` is a name of CLOCKS or a pair (clock_ln2, table).  Returns a dict of NumPy arrays with the fields
    of FIELDS (`energy_hist` only with hist=True): events_out - events_in accepted moves happened in n_segs seg_steps Metropolis steps,
    weight_out / (N^2 (N - 1) 2^24) is the Metropolis acceptance rate of the output under the last row.  A run may be cut at a segment
    boundary: feed `state`, `need_out` as need_in and `events_out` as events_in back in, with first_seg = the segments done so far and
    the rows that are left; best_energy / best_state / best_step of the whole are those of the FIRST piece with the smallest
    best_energy, its best_step moved by the steps before that piece, and n_uphill and n_flat add up.  ValueError for what the library
    refuses (N outside 2 .. 32, no chain, seg_steps outside 1 .. 2^31, a table_len above 128, a weight above 2^24, ...)."""
    s = _host_states(N, states)
    n, t = s.shape[0], _host_tables(tables)
    sd = _hop_seeds(seeds, n)
    ln2, ct = clock_tables(clock)
    need, events = _per_chain("need_in", need_in, n, np.uint64), _per_chain("events_in", events_in, n, np.int64)
    if n and t.shape[0]:  # the entries the device cannot look at, as the host entry refuses them
        if int(t.max()) > 1 << abi.NFOLD_WEIGHT_BITS:
            raise ValueError(f"a weight exceeds 2^{abi.NFOLD_WEIGHT_BITS}")
    if int(ct.max()) > 1 << abi.NFOLD_CLOCK_BITS:
        raise ValueError(f"a clock table entry exceeds 2^{abi.NFOLD_CLOCK_BITS}")
    if need is not None and need.size and int(need.max()) >= 1 << abi.NFOLD_NEED_BITS:
        raise ValueError(f"a need_in entry is not below 2^{abi.NFOLD_NEED_BITS}")
    if events is not None and events.size and int(events.min()) < 0:
        raise ValueError("events_in must be >= 0")
    res = _round_trip(_NFOLD, (N,), (t.shape[0], seg_steps, first_seg, t.shape[1], ln2), s,
                      lambda: (sd.view(np.int32), t.view(np.int32), ct.view(np.int32), None if need is None else need.view(np.int64), events),
                      lambda ts, tseeds, ttab, tclk, tneed, tev: nfold_device(N, ts, tseeds, ttab, seg_steps, first_seg=first_seg, clock=(ln2, tclk),
                                                                               need_in=tneed, events_in=tev, hist=hist))
    for k in ("need_out", "weight_out"):
        res[k] = res[k].view(np.uint64)
    return res


FIELDS_3D = FIELDS + ("flags",)


def _block3d(N, Q, n, n_segs, seg_steps, first_seg, table_len, clock_ln2):
    q = abi.Nfold3d()
    q.N, q.mode, q.n_queens, q.n_chains = int(N), abi.MODE_FULL3D, int(Q), int(n)
    q.n_segs, q.first_seg, q.seg_steps, q.table_len, q.clock_ln2 = int(n_segs), int(first_seg), int(seg_steps), int(table_len), int(clock_ln2)
    return q


_NFOLD3D = _Search(_block3d, abi.NFOLD3D_DTYPES, _lib.nfold3d_host, _lib.nfold3d_device, ("best_state",), True)


def nfold_queens_host(N, states, seeds, tables, seg_steps, Q=None, first_seg=0, clock="exp", need_in=None, events_in=None, hist=False):
    """mcq_nfold3d_host: the full_3d rule in the library's plain host code, which follows the definition (every (queen, cell) pair
    behind every event), NumPy in and out, no GPU.  Same result as nfold_queens, and it runs every shape (the kernel stops where a
    chain no longer fits the LDS: abi.nfold3d_lds_bytes)."""
    s = _host_queens(N, states, Q)
    n, t = s.shape[0], _host_tables(tables)
    ln2, ct = clock_tables(clock)
    width = t.shape[0] + 1
    ins = {"table": t, "clock_table": ct, "need_in": _per_chain("need_in", need_in, n, np.uint64), "events_in": _per_chain("events_in", events_in, n, np.int64)}
    return _host_call(_NFOLD3D, (N, _queens_of(N, Q)), s, (t.shape[0], seg_steps, first_seg, t.shape[1], ln2), {"energy_hist": (n, width)} if hist else {},
                      seeds, width, inputs=lambda: {k: a for k, a in ins.items() if a is not None and a.size})


def nfold_queens_device(N, states, seeds, tables, seg_steps, Q=None, first_seg=0, clock="exp", need_in=None, events_in=None, hist=False, out=None,
                        stream=None):
    """mcq_nfold3d_device on a torch uint8 tensor [n_chains][3 Q] or [n_chains][Q][3] of the current device (Q=None means N^2), enqueued
    on `stream` (default: torch's current stream).  ONE kernel whatever the number of segments is.  Asynchronous: nothing is copied back
    and nothing synchronises.  seeds, tables, clock, need_in and events_in are what nfold_device takes (a need is below 2^58 here, a row
    has up to abi.MAX_NFOLD3D_TABLE entries), and the entries of tensors are NOT checked.  `out` (optional) is the tensor the placements
    go to; it may be `states` itself (in place), default a new one.  Returns a dict of tensors with the fields of FIELDS_3D: those of
    nfold_device, `state` and `best_state` uint8 like `states`, plus `flags` int32[n_chains].  ValueError before any launch for what the
    library refuses, a chain above the LDS of a workgroup among it (abi.nfold3d_lds_bytes(N, Q) > abi.MAX_NFOLD3D_LDS)."""
    n, Qn = _device_queens("nfold_queens_device", N, states, Q)
    return _enqueue(_NFOLD3D, "nfold_queens_device", (N, Qn), n, states, seeds, tables, seg_steps, first_seg, clock, need_in, events_in, hist, out, stream)


def nfold_queens(N, states, seeds, tables, seg_steps, Q=None, first_seg=0, clock="exp", need_in=None, events_in=None, hist=False):
    """The n-fold way of full_3d placements on the GPU: `states` is uint8[n_chains][3 Q] or [n_chains][Q][3] (Q triples (i, j, k); Q=None
    means N^2), bytes >= N are clamped to N - 1; `seeds` is uint32[n_chains]; `tables` holds one weight row per segment
    (weight_tables(betas, abi.MAX_NFOLD3D_TABLE)) and every segment lasts seg_steps Metropolis steps of the reference's default move, a
    uniform queen to a uniform cell that holds no queen; `clock` is a name of CLOCKS or a pair (clock_ln2, table).  Returns a dict of
    NumPy arrays with the fields of FIELDS_3D (`energy_hist` only with hist=True): weight_out / (Q (N^3 - Q) 2^24) is the Metropolis
    acceptance rate of the output under the last row; flags bit 0 (abi.NFOLD3D_REPEATED) marks an input with two queens in one cell, which
    is recounted and handed back unmoved.  A run may be cut as nfold_states says.  A shape whose chain is above the LDS of a workgroup
    (abi.nfold3d_lds_bytes(N, Q) > abi.MAX_NFOLD3D_LDS: N = 32 runs up to Q = 8 470 on the device) is run by nfold_queens_host, which
    gives the same result.  ValueError for what the library refuses (N outside 2 .. 32, Q outside 2 .. N^3 - 1, no chain, seg_steps
    outside 1 .. 2^31, a table_len above 512, a weight above 2^24, ...)."""
    s = _host_queens(N, states, Q)
    n, t = s.shape[0], _host_tables(tables)
    sd = _hop_seeds(seeds, n)
    ln2, ct = clock_tables(clock)
    need, events = _per_chain("need_in", need_in, n, np.uint64), _per_chain("events_in", events_in, n, np.int64)
    kw = dict(Q=Q, first_seg=first_seg, hist=hist)
    if n and abi.MIN_N <= int(N) <= abi.MAX_N_QUENCH3D and abi.nfold3d_lds_bytes(N, Q) > abi.MAX_NFOLD3D_LDS:
        return nfold_queens_host(N, s, sd, t, seg_steps, clock=(ln2, ct), need_in=need, events_in=events, **kw)
    if n and t.shape[0]:  # the entries the device cannot look at, as the host entry refuses them
        if int(t.max()) > 1 << abi.NFOLD_WEIGHT_BITS:
            raise ValueError(f"a weight exceeds 2^{abi.NFOLD_WEIGHT_BITS}")
    if int(ct.max()) > 1 << abi.NFOLD_CLOCK_BITS:
        raise ValueError(f"a clock table entry exceeds 2^{abi.NFOLD_CLOCK_BITS}")
    if need is not None and need.size and int(need.max()) >= 1 << abi.NFOLD3D_NEED_BITS:
        raise ValueError(f"a need_in entry is not below 2^{abi.NFOLD3D_NEED_BITS}")
    if events is not None and events.size and int(events.min()) < 0:
        raise ValueError("events_in must be >= 0")
    res = _round_trip(_NFOLD3D, (N, _queens_of(N, Q)), (t.shape[0], seg_steps, first_seg, t.shape[1], ln2), s,
                      lambda: (sd.view(np.int32), t.view(np.int32), ct.view(np.int32), None if need is None else need.view(np.int64), events),
                      lambda ts, tseeds, ttab, tclk, tneed, tev: nfold_queens_device(N, ts, tseeds, ttab, seg_steps, clock=(ln2, tclk), need_in=tneed,
                                                                                      events_in=tev, **kw))
    for k in ("need_out", "weight_out"):
        res[k] = res[k].view(np.uint64)
    return res


def anneal_nfold(N, n_steps, init_mode, schedule_params, seeds, seg_steps=1000, clock="exp", hist=False, mcmc_type="board", Q=None):
    """Every chain of `seeds` for n_steps Metropolis steps of the n-fold way under one beta schedule, as ONE launch of n_steps /
    seg_steps segments: beta of segment s is abi.beta_values(schedule_params, n_steps)[s seg_steps], the reference's schedule read at
    the segment's first step and held over the segment.  n_steps must be a multiple of seg_steps.

    `init_mode` is an init mode of the reference ("random", "latin", "klarner": the placements are those of start_chains(N, 0,
    init_mode, ...), the reference's own initial state of chain seeds[r], as anneal_heatbath obtains them) or a uint8 array
    [n_chains][N*N] of placements.  Returns the dict of nfold_states (with hist=True `energy_hist` int32[n_chains][n_segs + 1]) plus
    `betas`, float64[n_segs].  mcmc_type="full_3d" runs full_3d placements of Q queens (default N^2) through nfold_queens instead: the
    initial placements are those of start_chains(..., mcmc_type="full_3d", Q=Q), or a uint8 array [n_chains][3 Q].  ValueError before
    anything is launched: an n_steps that is negative or no multiple of seg_steps, a list of schedules, a negative beta, an unknown
    clock, init mode or mcmc_type, placements of another shape."""
    n_steps, seg_steps = int(n_steps), int(seg_steps)
    if mcmc_type not in ("board", "full_3d"):
        raise ValueError(f"Unknown mcmc_type {mcmc_type!r}: anneal_nfold runs \"board\" and \"full_3d\"")
    cube = mcmc_type == "full_3d"
    if seg_steps < 1 or seg_steps > 1 << 31:
        raise ValueError(f"seg_steps out of range [1, 2^31]: {seg_steps}")
    if n_steps < 0 or n_steps % seg_steps:
        raise ValueError(f"n_steps must be a non-negative multiple of seg_steps = {seg_steps}, got {n_steps}")
    if isinstance(schedule_params, (list, tuple)):
        raise ValueError("anneal_nfold runs one schedule")
    clock = clock_tables(clock)
    sd = np.asarray(seeds)
    if sd.size and (sd.min() < 0 or sd.max() > 2**32 - 1):
        raise ValueError("Seed must be between 0 and 2**32 - 1")
    sd = _hop_seeds(sd, sd.size)
    n = len(sd)
    betas = np.ascontiguousarray(abi.beta_values(schedule_params, n_steps)[::seg_steps])
    tables = weight_tables(betas, abi.MAX_NFOLD3D_TABLE if cube else abi.MAX_NFOLD_TABLE)
    if not (abi.MIN_N <= int(N) <= abi.MAX_N_QUENCH_PAIRS):
        raise ValueError(f"N out of range [{abi.MIN_N}, {abi.MAX_N_QUENCH_PAIRS}]: {N}")
    Qn = _queens_of(N, Q)
    if cube and not 2 <= Qn <= int(N) ** 3 - 1:
        raise ValueError(f"n_queens out of range [2, N^3 - 1 = {int(N) ** 3 - 1}]: {Qn}")
    width = 3 * Qn if cube else int(N) * int(N)
    if isinstance(init_mode, str):
        from . import experiments as _ex

        if init_mode not in abi.INIT:
            raise ValueError(f"Unknown init_mode {init_mode}")
        first, _ = _ex.start_chains(N, 0, init_mode, schedule_params, sd, mcmc_type=mcmc_type, trace=False, states=True, **({"Q": Qn} if cube else {}))
        start = np.ascontiguousarray(first["final_state"], dtype=np.uint8).reshape(n, -1)
    else:
        start = _host_queens(N, init_mode, Qn) if cube else _host_states(N, init_mode)
    if start.shape != (n, width):
        raise ValueError(f"init_mode must be uint8[{n}][{width}] (one placement per seed), got {start.shape}")
    if cube:
        res = nfold_queens(N, start, sd, tables, seg_steps, Q=Qn, clock=clock, hist=hist)
    else:
        res = nfold_states(N, start, sd, tables, seg_steps, clock=clock, hist=hist)
    res["betas"] = betas
    return res
