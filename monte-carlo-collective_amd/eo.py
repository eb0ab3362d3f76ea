"""Extremal optimisation, the tau-EO of Boettcher and Percus, of board placements (include/mcq.h: mcq_eo, where the rule is stated;
csrc/mcq_eo.hip) and of full_3d placements (mcq_eo3d; csrc/mcq_eo3d.hip).

NOT a mode of the reference, never a default, and labelled as such like Philox, the heat baths, the searches and the n-fold way.
Every search of quench.py chooses a move by the energy change it causes and the samplers choose by a temperature.  This one ranks
the N^2 columns by their local badness lambda(c) = a(c, h(c)), the number of queens that attack the column's queen, draws a rank j
from a power law P(j) ~ (j + 1)^-tau and moves the column at that rank unconditionally, to its best other height (move="best") or
to a random one (move="random").  No temperature, no memory, no acceptance test, one parameter.  The rule is integer-exact, so the
library's host code, the kernel and a NumPy restatement (tests/eo_util.py) agree bit for bit.  Boards, N = 2 .. 32.

rank_table gives the table of a tau; eo_states_host, eo_device and eo_states run a call.  A run cut into calls is the unbroken run
when `state`, `best_energy` -> best_floor and first_iter are carried over; there is nothing else to carry.

The full_3d form ranks the Q queens of a placement of triples instead, lambda(q) = the number of queens that attack queen q, and
moves the queen at the drawn rank to the free cell of the cube with the fewest attackers (move="best") or to a uniform free cell
(move="random"): eo_queens_host, eo_queens_device and eo_queens, with rank_table(N, tau, Q) for their table.  The restatement is
tests/eo3d_util.py; N = 2 .. 32, Q = 2 .. N^3 - 1, every shape on the device.  A run is cut in the same way.
"""
import numpy as np

from . import _lib, abi
from .quench import (_Search, _device_call, _device_queens, _device_states, _hop_seeds, _host_call, _host_queens, _host_states, _queens_of,
                     _round_trip)

FIELDS = ("state", "energy_in", "energy_out", "best_energy", "best_iter", "best_state", "n_moves", "n_uphill", "n_flat", "n_free", "n_idle",
          "energy_hist")
MOVES = ("best", "random")


def rank_table(N, tau, Q=None):
    """The rank table of a tau (include/mcq.h, mcq_eo rule, item 4) as uint32[N^2 - 1]: with P(j) = (j + 1)^-tau / sum over the ranks
    j = 0 .. N^2 - 1, entry i = min(2^32 - 1, floor(2^32 (P(0) + ... + P(i)))), NumPy's float64 arithmetic.  tau = 0 is the uniform
    draw over all columns, tau = np.inf gives 2^32 - 1 everywhere: always the worst column.  With Q (full_3d, mcq_eo3d rule, item 4)
    the ranks are those of Q queens: uint32[Q - 1], 2 <= Q <= N^3 - 1."""
    N, tau = int(N), float(tau)
    if Q is None:
        if not abi.MIN_N <= N <= abi.MAX_N_QUENCH_PAIRS:
            raise ValueError(f"N out of range [{abi.MIN_N}, {abi.MAX_N_QUENCH_PAIRS}]: {N}")
        ranks = N * N
    else:
        ranks = int(Q)
        if not abi.MIN_N <= N <= abi.MAX_N_QUENCH3D:
            raise ValueError(f"N out of range [{abi.MIN_N}, {abi.MAX_N_QUENCH3D}]: {N}")
        if not 2 <= ranks <= N ** 3 - 1:
            raise ValueError(f"Q out of range [2, N^3 - 1 = {N ** 3 - 1}]: {ranks}")
    if not tau >= 0.0:
        raise ValueError(f"tau must be >= 0 (np.inf: always the worst column), got {tau}")
    p = np.power(np.arange(1, ranks + 1, dtype=np.float64), -tau)
    cum = np.cumsum(p / p.sum())[:-1]
    return np.minimum(np.floor(cum * 4294967296.0), 4294967295.0).astype(np.uint32)


def _move(move):
    if move not in MOVES:
        raise ValueError(f"Unknown move {move!r}: extremal optimisation has the moves {MOVES}")
    return MOVES.index(move)


def _block(N, n, n_iters, first_iter, move, n_ranks):
    q = abi.Eo()
    q.N, q.mode, q.n_chains, q.n_iters, q.first_iter, q.move, q.n_ranks = int(N), abi.MODE_BOARD, int(n), int(n_iters), int(first_iter), int(move), int(n_ranks)
    return q


_EO = _Search(_block, abi.EO_DTYPES, _lib.eo_host, _lib.eo_device, ("best_state",), True)


def _host_ranks(N, tau, rank_cdf, Q=None):
    """The table of a call as uint32[n_ranks]: the caller's, or rank_table(N, tau, Q)."""
    if rank_cdf is None:
        return rank_table(N, tau, Q)
    t = np.ascontiguousarray(rank_cdf, dtype=np.uint32)
    if t.ndim != 1:
        raise ValueError(f"rank_cdf must be uint32[n_ranks] (rank_table), got {t.shape}")
    return t


def _host_floor(best_floor, n):
    if best_floor is None:
        return None
    f = np.ascontiguousarray(best_floor, dtype=np.int32).reshape(-1)
    if f.shape[0] != n:
        raise ValueError(f"best_floor must be int32[n_chains = {n}], got {np.shape(best_floor)}")
    return f


def eo_states_host(N, states, seeds, n_iters, tau=1.4, move="best", rank_cdf=None, first_iter=0, best_floor=None, hist=False):
    """mcq_eo_host: extremal optimisation in the library's plain host code, NumPy in and out, no GPU.  Same result as eo_states."""
    s = _host_states(N, states)
    n, width, mv = s.shape[0], max(int(n_iters), 0) + 1, _move(move)
    ins = {"rank_cdf": _host_ranks(N, tau, rank_cdf), "best_floor": _host_floor(best_floor, n)}
    return _host_call(_EO, (N,), s, (n_iters, first_iter, mv, ins["rank_cdf"].shape[0]), {"energy_hist": (n, width)} if hist else {}, seeds, width,
                      inputs=lambda: {k: a for k, a in ins.items() if a is not None and a.size})


def eo_device(N, states, seeds, n_iters, tau=1.4, move="best", rank_cdf=None, first_iter=0, best_floor=None, hist=False, out=None, stream=None):
    """mcq_eo_device on a torch uint8 tensor [n_chains][N*N] of the current device (e.g. DeviceRun.t["best_state"]), enqueued on
    `stream` (default: torch's current stream).  ONE kernel whatever n_iters is.  Asynchronous: nothing is copied back and nothing
    synchronises, so the results are valid once the stream has passed the call.  `seeds` is an int32 or uint32 tensor [n_chains] on the
    device (the seeds' 32 bits, whatever the sign) or a NumPy array / list, which is uploaded on the stream; `rank_cdf` is a uint32 NumPy
    array [n_ranks] or an int32 tensor of its bits on the device (default: rank_table(N, tau), uploaded), whose entries are NOT checked:
    the rule counts the entries <= x0 of any table; `best_floor` is an int32 tensor [n_chains], the best_energy of an earlier call.
    `out` (optional) is the tensor the final placements go to; it may be `states` itself (in place), default a new one.  Returns a
    dict of tensors with the fields of FIELDS: `state` and `best_state` uint8 like `states`; `energy_in`, `energy_out`, `best_energy`
    int32[n_chains]; `best_iter`, `n_moves`, `n_uphill`, `n_flat`, `n_free`, `n_idle` int64[n_chains]; with hist=True `energy_hist`
    int32[n_chains][n_iters + 1]."""
    import torch

    from .heatbath import _upload

    n, width, mv = _device_states("eo_device", N, states), max(int(n_iters), 0) + 1, _move(move)
    dev = states.device
    st = torch.cuda.current_stream(dev) if stream is None else stream
    with torch.cuda.device(dev), torch.cuda.stream(st):
        if isinstance(rank_cdf, torch.Tensor):
            if not (rank_cdf.device == dev and rank_cdf.is_contiguous() and rank_cdf.dim() == 1
                    and rank_cdf.dtype in (torch.int32, getattr(torch, "uint32", torch.int32))):
                raise ValueError("eo_device takes rank_cdf as a contiguous int32 or uint32 tensor [n_ranks] on the device of states")
            ranks, n_ranks = rank_cdf, int(rank_cdf.shape[0])
        else:
            t = _host_ranks(N, tau, rank_cdf)
            ranks, n_ranks = (_upload(t.view(np.int32), dev) if t.size else None), int(t.shape[0])
        if not isinstance(seeds, torch.Tensor):
            seeds = _upload(_hop_seeds(seeds, n).view(np.int32), dev)
        if best_floor is not None and not (isinstance(best_floor, torch.Tensor) and best_floor.device == dev and best_floor.is_contiguous()
                                           and best_floor.dtype == torch.int32 and tuple(best_floor.shape) == (n,)):
            raise ValueError(f"eo_device takes best_floor as a contiguous int32 tensor [n_chains = {n}] on the device of states")
        ins = {k: t for k, t in (("rank_cdf", ranks), ("best_floor", best_floor)) if t is not None and t.numel()}
        res = _device_call(_EO, "eo_device", (N,), n, states, (n_iters, first_iter, mv, n_ranks), {"energy_hist": (n, width)} if hist else {}, seeds, width,
                           inputs=lambda: ins, out=out, stream=st)
        for t in (seeds,) + tuple(ins.values()):
            t.record_stream(st)  # (the kernel reads them after this call has returned)
    return res


def to_numpy(res):
    """The dict eo_device returned, as NumPy arrays.  The stream must have passed the call."""
    return {k: t.cpu().numpy() for k, t in res.items()}


def eo_states(N, states, seeds, n_iters, tau=1.4, move="best", rank_cdf=None, first_iter=0, best_floor=None, hist=False):
    """Extremal optimisation of board placements on the GPU: `states` is uint8[n_chains][N*N] (one board of N*N heights is taken as one
    chain), bytes >= N are clamped to N - 1; `seeds` is uint32[n_chains].  No descent runs first.  Each of the n_iters iterations orders
    the columns by the number of queens that attack their queen, the worst first and ties by a random rotation, draws a position from
    `rank_cdf` (default rank_table(N, tau): P(j) ~ (j + 1)^-tau) and moves that column -- to the height with the fewest attackers other
    than its own (move="best"; ties by a random rotation) or to a uniform other height (move="random") --, whatever that does to the
    energy.  A chain at energy 0 idles.  Returns a dict of NumPy arrays with the fields of FIELDS (`energy_hist` only with hist=True);
    best_state is the best placement the call saw, the input when best_iter = 0.  A run may be cut: feed `state` back in with first_iter
    = the iterations done so far and best_floor = the best_energy of the piece before; the counters of the pieces add up, and
    best_state / best_iter of the whole are those of the LAST piece with best_iter > 0.  ValueError for what the library refuses (N
    outside 2 .. 32, no chain, a negative n_iters or first_iter, more than N^2 - 1 ranks, a table that decreases) and for an unknown
    move."""
    s = _host_states(N, states)
    n, mv = s.shape[0], _move(move)
    sd, t, bf = _hop_seeds(seeds, n), _host_ranks(N, tau, rank_cdf), _host_floor(best_floor, n)
    if t.size > 1 and (t[1:] < t[:-1]).any():  # the entries the device cannot look at, as the host entry refuses them
        raise ValueError("rank_cdf must not decrease")
    return _round_trip(_EO, (N,), (n_iters, first_iter, mv, t.shape[0]), s, lambda: (sd.view(np.int32), t.view(np.int32) if t.size else None, bf),
                       lambda ts, tseeds, tranks, tfloor: eo_device(N, ts, tseeds, n_iters, move=move, first_iter=first_iter, best_floor=tfloor, hist=hist,
                                                                    rank_cdf=tranks if tranks is not None else t))


FIELDS_QUEENS = FIELDS + ("flags",)


def _block_queens(N, Q, n, n_iters, first_iter, move, n_ranks):
    q = abi.Eo3d()
    q.N, q.n_queens, q.n_chains, q.n_iters, q.first_iter, q.move, q.n_ranks = int(N), int(Q), int(n), int(n_iters), int(first_iter), int(move), int(n_ranks)
    return q


_EO3D = _Search(_block_queens, abi.EO3D_DTYPES, _lib.eo3d_host, _lib.eo3d_device, ("best_state",), True)


def _queens_ranks(N, Q, tau, rank_cdf):
    """_host_ranks for the full_3d form.  The default table needs a shape in range; outside it an empty table goes to the library, which
    refuses the shape with its own text."""
    Qn = _queens_of(N, Q)
    if rank_cdf is None and not (abi.MIN_N <= int(N) <= abi.MAX_N_QUENCH3D and 2 <= Qn <= int(N) ** 3 - 1):
        return np.zeros(0, dtype=np.uint32)
    return _host_ranks(N, tau, rank_cdf, Qn)


def eo_queens_host(N, states, seeds, n_iters, Q=None, tau=1.4, move="best", rank_cdf=None, first_iter=0, best_floor=None, hist=False):
    """mcq_eo3d_host: extremal optimisation of full_3d placements in the library's plain host code, NumPy in and out, no GPU.  Same
    result as eo_queens."""
    s, Qn = _host_queens(N, states, Q), _queens_of(N, Q)
    n, width, mv = s.shape[0], max(int(n_iters), 0) + 1, _move(move)
    ins = {"rank_cdf": _queens_ranks(N, Q, tau, rank_cdf), "best_floor": _host_floor(best_floor, n)}
    return _host_call(_EO3D, (N, Qn), s, (n_iters, first_iter, mv, ins["rank_cdf"].shape[0]), {"energy_hist": (n, width)} if hist else {}, seeds, width,
                      inputs=lambda: {k: a for k, a in ins.items() if a is not None and a.size})


def eo_queens_device(N, states, seeds, n_iters, Q=None, tau=1.4, move="best", rank_cdf=None, first_iter=0, best_floor=None, hist=False, out=None,
                     stream=None):
    """mcq_eo3d_device on a torch uint8 tensor [n_chains][3 Q] or [n_chains][Q][3] of the current device (e.g. DeviceRun.t["best_state"]
    of a full_3d run; Q=None means N^2), enqueued on `stream` (default: torch's current stream).  ONE kernel whatever n_iters is.
    Asynchronous: nothing is copied back and nothing synchronises, so the results are valid once the stream has passed the call.
    `seeds`, `rank_cdf` and `best_floor` are as eo_device takes them (the default table is rank_table(N, tau, Q), uploaded).  `out`
    (optional) is the tensor the final placements go to; it may be `states` itself (in place), default a new one.  Returns a dict of
    tensors with the fields of FIELDS_QUEENS: `state` and `best_state` uint8 like `states`; `energy_in`, `energy_out`, `best_energy`,
    `flags` int32[n_chains]; `best_iter`, `n_moves`, `n_uphill`, `n_flat`, `n_free`, `n_idle` int64[n_chains]; with hist=True
    `energy_hist` int32[n_chains][n_iters + 1]."""
    import torch

    from .heatbath import _upload

    (n, Qn), width, mv = _device_queens("eo_queens_device", N, states, Q), max(int(n_iters), 0) + 1, _move(move)
    dev = states.device
    st = torch.cuda.current_stream(dev) if stream is None else stream
    with torch.cuda.device(dev), torch.cuda.stream(st):
        if isinstance(rank_cdf, torch.Tensor):
            if not (rank_cdf.device == dev and rank_cdf.is_contiguous() and rank_cdf.dim() == 1
                    and rank_cdf.dtype in (torch.int32, getattr(torch, "uint32", torch.int32))):
                raise ValueError("eo_queens_device takes rank_cdf as a contiguous int32 or uint32 tensor [n_ranks] on the device of states")
            ranks, n_ranks = rank_cdf, int(rank_cdf.shape[0])
        else:
            t = _queens_ranks(N, Q, tau, rank_cdf)
            ranks, n_ranks = (_upload(t.view(np.int32), dev) if t.size else None), int(t.shape[0])
        if not isinstance(seeds, torch.Tensor):
            seeds = _upload(_hop_seeds(seeds, n).view(np.int32), dev)
        if best_floor is not None and not (isinstance(best_floor, torch.Tensor) and best_floor.device == dev and best_floor.is_contiguous()
                                           and best_floor.dtype == torch.int32 and tuple(best_floor.shape) == (n,)):
            raise ValueError(f"eo_queens_device takes best_floor as a contiguous int32 tensor [n_chains = {n}] on the device of states")
        ins = {k: t for k, t in (("rank_cdf", ranks), ("best_floor", best_floor)) if t is not None and t.numel()}
        res = _device_call(_EO3D, "eo_queens_device", (N, Qn), n, states, (n_iters, first_iter, mv, n_ranks), {"energy_hist": (n, width)} if hist else {},
                           seeds, width, inputs=lambda: ins, out=out, stream=st)
        for t in (seeds,) + tuple(ins.values()):
            t.record_stream(st)  # (the kernel reads them after this call has returned)
    return res


def eo_queens(N, states, seeds, n_iters, Q=None, tau=1.4, move="best", rank_cdf=None, first_iter=0, best_floor=None, hist=False):
    """Extremal optimisation of full_3d placements on the GPU: `states` is uint8[n_chains][3 Q] or [n_chains][Q][3] (Q triples (i, j, k);
    Q=None means N^2), bytes >= N are clamped to N - 1; `seeds` is uint32[n_chains].  No descent runs first.  Each of the n_iters
    iterations orders the queens by the number of queens that attack them, the worst first and ties by a random rotation, draws a
    position from `rank_cdf` (default rank_table(N, tau, Q): P(j) ~ (j + 1)^-tau) and moves that queen -- to the free cell of the cube
    with the fewest attackers (move="best"; ties by a random rotation of the cells) or to a uniform free cell (move="random") --,
    whatever that does to the energy.  A chain at energy 0 idles.  Returns a dict of NumPy arrays with the fields of FIELDS_QUEENS
    (`energy_hist` only with hist=True); best_state is the best placement the call saw, the input when best_iter = 0; flags bit 0
    (abi.EO3D_REPEATED) marks an input with two queens in one cell, which is recounted and handed back unmoved.  A run may be cut as
    eo_states says.  Every shape runs on the device (abi.eo3d_lds_bytes).  ValueError for what the library refuses (N outside 2 .. 32,
    Q outside 2 .. N^3 - 1, no chain, a negative n_iters or first_iter, more than Q - 1 ranks, a table that decreases) and for an
    unknown move."""
    s, Qn = _host_queens(N, states, Q), _queens_of(N, Q)
    n, mv = s.shape[0], _move(move)
    sd, t, bf = _hop_seeds(seeds, n), _queens_ranks(N, Q, tau, rank_cdf), _host_floor(best_floor, n)
    if t.size > 1 and (t[1:] < t[:-1]).any():  # the entries the device cannot look at, as the host entry refuses them
        raise ValueError("rank_cdf must not decrease")
    return _round_trip(_EO3D, (N, Qn), (n_iters, first_iter, mv, t.shape[0]), s, lambda: (sd.view(np.int32), t.view(np.int32) if t.size else None, bf),
                       lambda ts, tseeds, tranks, tfloor: eo_queens_device(N, ts, tseeds, n_iters, Q=Q, move=move, first_iter=first_iter, best_floor=tfloor,
                                                                           hist=hist, rank_cdf=tranks if tranks is not None else t))
