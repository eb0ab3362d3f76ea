"""Quench: the deterministic zero-temperature descent of board placements to a local minimum (include/mcq.h: mcq_quench, where the rule
is stated; csrc/mcq_quench.hip).

NOT a mode of the reference -- it ships conflicts_for_position (mcmc_board.py:147-193) and never uses it --, never a default, and
labelled as such like Philox, replica exchange and population annealing.  What a sweep hands back (best_state, final_state, the
competition board) is whatever a thermal chain last held; the quench says whether that placement is a local minimum under
single-height moves, what the minimum below it is, recounts its energy on the device independently of the sweep, and returns the
per-column conflict map.  Boards: N = 2 .. 128 (quench_states*, quench_device).

quench_pairs, quench_pairs_device and quench_pairs_host go one neighbourhood further (include/mcq.h: mcq_quench_pairs;
csrc/mcq_quench_pairs.hip): the descent also takes moves of two aligned columns at once and ends on a placement that no single move
and no pair move lowers.  Boards, N = 2 .. 32; opt-in like everything here.

hop_states, hop_device and hop_host go on from a minimum (include/mcq.h: mcq_hop; csrc/mcq_hop.hip): basin hopping, that is a kick of
a few columns, the single-move or the pair-move descent again, and the new minimum kept when it is no worse.  A whole run of hops is
one launch.  Boards, N = 2 .. 32; opt-in like everything here.

tabu_states, tabu_device and tabu_host walk on from a minimum instead of falling back onto it (include/mcq.h: mcq_tabu;
csrc/mcq_tabu.hip): tabu search, that is the best admissible single-height move of a conflicting column in every iteration, also when
it raises the energy, with the height left forbidden for a while.  A whole run is one launch.  Boards, N = 2 .. 32; opt-in like
everything here.

relink_states, relink_device and relink_host combine two placements (include/mcq.h: mcq_relink; csrc/mcq_relink.hip): path relinking, that
is a walk from a placement towards a guide, one column at a time and always the cheapest remaining one, with the best placement met on
the way handed to the single-move or the pair-move descent.  board_images and nearest_image bring a guide into the one of its 16
symmetric images that is closest to the placement, and relink_pool runs rounds of relinking over a pool of placements, each slot with a
rolled partner.  A whole call is one launch.  Boards, N = 2 .. 32; opt-in like everything here.

full_3d placements have a rule and a kernel of their own (include/mcq.h: mcq_quench3d; csrc/mcq_quench3d.hip), N = 2 .. 32 and
2 <= Q <= N^3 - 1: quench_queens, quench_queens_device, quench_queens_host.  The same labels apply -- the reference ships
conflicts_for_queen (mcmc.py:185-226) and never calls it.

hop_queens, hop_queens_device and hop_queens_host go on from a full_3d minimum (include/mcq.h: mcq_hop3d; csrc/mcq_hop3d.hip): a kick
moves a few queens to free cells, the single-queen descent runs again, and the new minimum is kept when it is no worse; a whole run of
hops is one launch.  queens_of_boards carries board placements into the cube.  Opt-in like everything here.

tabu_queens, tabu_queens_device and tabu_queens_host walk on from a full_3d placement (include/mcq.h: mcq_tabu3d; csrc/mcq_tabu3d.hip):
the best admissible move of a conflicting queen to a free cell in every iteration, also when it raises the energy, with the cell left
forbidden for a while.  A whole run is one launch.  Opt-in like everything here.

relink_queens, relink_queens_device and relink_queens_host combine two full_3d placements (include/mcq.h: mcq_relink3d;
csrc/mcq_relink3d.hip): a walk towards the guide's set of cells, one queen at a time and always the cheapest remaining (queen, cell)
pair, with the best placement met on the way handed to the single-queen descent.  queens_images and nearest_queens_image bring a guide
into the one of its 48 images under the cube's symmetries that is closest to the placement, and relink_queens_pool runs rounds of
relinking over a pool.  A whole call is one launch.  Opt-in like everything here.
"""
import collections

import numpy as np

from . import _lib, abi

FIELDS = ("state", "energy_in", "energy_out", "n_moves", "n_passes", "conflicts")


def _block(N, n, max_passes):
    q = abi.Quench()
    q.N, q.mode, q.n_chains, q.max_passes = int(N), abi.MODE_BOARD, int(n), int(max_passes)
    return q


def _host_states(N, states):
    s = np.ascontiguousarray(states, dtype=np.uint8)
    N = int(N)
    if s.size == 0:
        return s.reshape(0, max(N, 0) ** 2)
    if s.ndim == 1 or s.shape == (N, N):  # one board
        s = s.reshape(1, -1)
    s = s.reshape(s.shape[0], -1)
    if abi.MIN_N <= N <= abi.MAX_N_BOARD and s.shape[1] != N * N:
        raise ValueError(f"states must be uint8[n_chains][{N * N}] (final_state layout of a board), got {s.shape}")
    return s


def _host_outputs(q, s, dtypes, shapes=None, skip=(), like=()):
    """The host outputs of a call on the placements `s`, allocated from a *_DTYPES table -- one entry per chain, or the shape `shapes`
    names; the fields in `skip` are left out -- with `state` and the uint8 arrays named in `like` shaped like s, and the block `q`
    pointed at all of them and at s."""
    out = {k: np.zeros_like(s) for k in ("state",) + tuple(like)}
    for k, dt in dtypes.items():
        if k not in skip:
            out[k] = np.zeros((shapes or {}).get(k, s.shape[0]), dtype=dt)
    q.state_in, q.state_out = s.ctypes.data, out["state"].ctypes.data
    for k in tuple(like) + tuple(dtypes):
        if k in out:
            setattr(q, k, out[k].ctypes.data)
    return out


def _device_tensor(fn, states):
    """ValueError unless `states` is what the wrapper `fn` takes: a contiguous uint8 tensor on the GPU."""
    import torch

    if not (isinstance(states, torch.Tensor) and states.is_cuda and states.dtype == torch.uint8 and states.is_contiguous()):
        raise ValueError(f"{fn} takes a contiguous uint8 tensor on the GPU")


def _device_states(fn, N, states):
    """The checks of a device tensor of boards, [n_chains][N*N]; returns n_chains."""
    _device_tensor(fn, states)
    n = int(states.shape[0]) if states.dim() == 2 else 0
    if states.dim() != 2 or (abi.MIN_N <= int(N) <= abi.MAX_N_BOARD and int(states.shape[1]) != int(N) * int(N)):
        raise ValueError(f"states must be uint8[n_chains][{int(N) * int(N)}] (final_state layout of a board), got {tuple(states.shape)}")
    return n


def _device_queens(fn, N, states, Q):
    """The checks of a device tensor of full_3d placements, [n_chains][3 Q] or [n_chains][Q][3]; returns (n_chains, Q)."""
    _device_tensor(fn, states)
    Qn = _queens_of(N, Q)
    ok = (states.dim() == 2 and int(states.shape[1]) == 3 * Qn) or (states.dim() == 3 and tuple(states.shape[1:]) == (Qn, 3))
    if states.dim() not in (2, 3) or (abi.MIN_N <= int(N) <= abi.MAX_N_QUENCH3D and Qn >= 2 and not ok):
        raise ValueError(f"states must be uint8[n_chains][{3 * Qn}] or [n_chains][{Qn}][3] (final_state layout of full_3d), got {tuple(states.shape)}")
    return int(states.shape[0]), Qn


def _device_out(out, states):
    """The tensor the placements go to: `out` when given (checked; it may be `states`), a new one otherwise."""
    import torch

    if out is None:
        return torch.empty_like(states)
    if out.shape != states.shape or out.dtype != torch.uint8 or out.device != states.device or not out.is_contiguous():
        raise ValueError("out must be a contiguous uint8 tensor of the shape and device of states")
    return out


# One search of this module: `block` builds its parameter block from (N, n_chains, ...) -- (N, Q, n_chains, ...) for full_3d --, `dtypes`
# is its *_DTYPES table, `host` and `device` are its entries in _lib, `like` names the placements it returns next to `state`, and
# `seeds` says whether it draws (a seed per chain and a history stride in the block).
_Search = collections.namedtuple("_Search", "block dtypes host device like seeds")
# the outputs with a row per chain, which a caller turns on: a call allocates those it is given a shape for
_ROWS = ("conflicts", "energy_hist", "tabu_out")
_QUENCH = _Search(_block, abi.QUENCH_DTYPES, _lib.quench_host, _lib.quench_device, (), False)


def _skip(d, shapes, figures):
    """The fields of d.dtypes a call leaves out: the rows without a shape, and with figures=False everything else as well."""
    return tuple(k for k in d.dtypes if k not in shapes and (k in _ROWS or not figures))


def _check_seeds(fn, seeds, n, dev):
    """ValueError unless `seeds` is what the device wrapper `fn` of a search takes: the seeds' 32 bits, whatever the sign."""
    import torch

    if not (isinstance(seeds, torch.Tensor) and seeds.device == dev and seeds.dtype in (torch.int32, getattr(torch, "uint32", torch.int32)) and seeds.is_contiguous()
            and tuple(seeds.shape) == (n,)):
        raise ValueError(f"{fn} takes seeds as a contiguous int32 or uint32 tensor [n_chains = {n}] on the device of states")


def _host_call(d, dims, s, args, shapes, seeds=None, width=0, inputs=None, figures=True):
    """The search `d` in the library's host code on the placements `s` (_host_states, _host_queens): the seeds checked, the block from
    d.block(*dims, n_chains, *args), _host_outputs with the rows `shapes` names, and the call.  `inputs` (optional) is called behind the
    seeds' check and gives {field: array} of what else the block points at; `width` is the history stride.  Returns the outputs."""
    n = s.shape[0]
    if d.seeds:
        seeds = _hop_seeds(seeds, n)
    q = d.block(*dims, n, *args)
    out = _host_outputs(q, s, d.dtypes, shapes, _skip(d, shapes, figures), like=d.like if figures else ())
    keep = dict(inputs() if inputs else {}, **({"seeds": seeds} if d.seeds else {}))  # referenced until the library has returned
    for k, a in keep.items():
        setattr(q, k, a.ctypes.data)
    if d.seeds:
        q.hist_stride = width
    d.host(q)
    return out


def _device_call(d, fn, dims, n, states, args, shapes, seeds=None, width=0, inputs=None, figures=True, out=None, stream=None):
    """The search `d` enqueued for the device wrapper `fn` on the checked tensor `states` of n chains, on `stream` (default: torch's
    current stream) and the device of states: _host_call's steps with tensors -- `state` is _device_out's, a field of d.dtypes gets the
    signed torch type of its width --, and nothing is copied back or waited for.  Returns the dict of result tensors."""
    import torch

    dev = states.device
    if d.seeds:
        _check_seeds(fn, seeds, n, dev)
    ins = dict(inputs() if inputs else {}, **({"seeds": seeds} if d.seeds else {}))
    st = torch.cuda.current_stream(dev) if stream is None else stream
    tdt = {np.int32: torch.int32, np.int64: torch.int64, np.uint16: torch.int16, np.uint64: torch.int64}
    skip = _skip(d, shapes, figures)
    with torch.cuda.device(dev), torch.cuda.stream(st):
        q = d.block(*dims, n, *args)
        res = {"state": _device_out(out, states)}
        for k in d.like if figures else ():
            res[k] = torch.empty_like(states)
        for k, dt in d.dtypes.items():
            if k not in skip:
                res[k] = torch.empty(shapes.get(k, n), dtype=tdt[dt], device=dev)
        q.state_in, q.state_out = states.data_ptr(), res["state"].data_ptr()
        for k, t in list(res.items())[1:] + list(ins.items()):
            setattr(q, k, t.data_ptr())
        if d.seeds:
            q.hist_stride = width
        d.device(q, st)
    return res


def _round_trip(d, dims, args, s, arrays, call):
    """What the NumPy wrappers of the device searches share: no chain is refused by the library's host entry, the placements `s` and the
    host arrays `arrays()` gives (None stays None) go to the current device, `call` hands them to the device wrapper, the stream is
    waited for and the results come back as NumPy arrays, the placements in the shape of s."""
    import torch

    if s.shape[0] == 0:
        d.host(d.block(*dims, 0, *args))  # raises the library's refusal
    dev = torch.device("cuda", torch.cuda.current_device())
    res = call(*(None if a is None else torch.from_numpy(a).to(dev) for a in (s,) + tuple(arrays())))
    torch.cuda.current_stream(dev).synchronize()
    out = (tabu_to_numpy if "tabu_out" in d.dtypes else to_numpy)(res)
    for k in ("state",) + d.like:
        if k in out:
            out[k] = out[k].reshape(s.shape)
    return out


def quench_states_host(N, states, max_passes=0, conflicts=True):
    """mcq_quench_host: the rule in the library's plain host code, NumPy in and out, no GPU.  Same result as quench_states."""
    s = _host_states(N, states)
    return _host_call(_QUENCH, (N,), s, (max_passes,), {"conflicts": s.shape} if conflicts else {})


def quench_device(N, states, max_passes=0, out=None, conflicts=True, stream=None):
    """mcq_quench_device on a torch uint8 tensor [n_chains][N*N] of the current device (e.g. DeviceRun.t["best_state"]), enqueued on
    `stream` (default: torch's current stream).  Asynchronous: nothing is copied back and nothing synchronises, so the results are valid
    once the stream has passed the call.  `out` (optional) is the tensor the placements go to; it may be `states` itself (in place),
    default a new one.  Returns a dict of tensors: `state` uint8 like `states`, `energy_in` (the recount of the input), `energy_out`,
    `n_moves`, `n_passes` int32[n_chains] and, unless conflicts=False, `conflicts` int16[n_chains][N*N] (the uint16 counts a(c, h(c)) of the
    output; at most 4 (N - 1), so the sign bit is never set)."""
    n = _device_states("quench_device", N, states)
    return _device_call(_QUENCH, "quench_device", (N,), n, states, (max_passes,), {"conflicts": tuple(states.shape)} if conflicts else {}, out=out, stream=stream)


def quench_states(N, states, max_passes=0, conflicts=True):
    """Quench board placements on the GPU: `states` is uint8[n_chains][N*N] (the final_state / best_state layout; one board of N*N
    heights is taken as one chain), bytes >= N are clamped to N - 1.  max_passes = 0 runs until a pass makes no move.  Returns a dict of
    NumPy arrays: `state` (the placements after the descent), `energy_in` (the energy of the input, recounted on the device),
    `energy_out`, `n_moves`, `n_passes` int32[n_chains], and `conflicts` uint16[n_chains][N*N], the number of queens attacking each
    column's queen in the output (its sum is 2 energy_out).  A placement with n_moves == 0 was a local minimum already.
    ValueError for what the library refuses (N outside 2 .. 128, no chain, a negative max_passes)."""
    return _round_trip(_QUENCH, (N,), (max_passes,), _host_states(N, states), lambda: (),
                       lambda t: quench_device(N, t, max_passes=max_passes, conflicts=conflicts))


def to_numpy(res):
    """The dict quench_device returned, as NumPy arrays (conflicts as uint16).  The stream must have passed the call."""
    out = {k: t.cpu().numpy() for k, t in res.items()}
    if "conflicts" in out:
        out["conflicts"] = out["conflicts"].view(np.uint16)
    return out


FIELDS_PAIRS = ("state", "energy_in", "energy_single", "energy_out", "n_moves", "n_pair_moves", "n_rounds", "certified", "conflicts")


def _block_pairs(N, n, max_rounds):
    q = abi.QuenchPairs()
    q.N, q.mode, q.n_chains, q.max_rounds = int(N), abi.MODE_BOARD, int(n), int(max_rounds)
    return q


_PAIRS = _Search(_block_pairs, abi.QUENCH_PAIRS_DTYPES, _lib.quench_pairs_host, _lib.quench_pairs_device, (), False)


def quench_pairs_host(N, states, max_rounds=0, conflicts=True):
    """mcq_quench_pairs_host: the pair-move rule in the library's plain host code, NumPy in and out, no GPU.  Same result as
    quench_pairs."""
    s = _host_states(N, states)
    return _host_call(_PAIRS, (N,), s, (max_rounds,), {"conflicts": s.shape} if conflicts else {})


def quench_pairs_device(N, states, max_rounds=0, out=None, conflicts=True, stream=None):
    """mcq_quench_pairs_device on a torch uint8 tensor [n_chains][N*N] of the current device (e.g. DeviceRun.t["best_state"]), enqueued
    on `stream` (default: torch's current stream).  Asynchronous like quench_device: nothing is copied back and nothing synchronises.
    `out` (optional) is the tensor the placements go to; it may be `states` itself (in place), default a new one.  Returns a dict of
    tensors: `state` uint8 like `states`; `energy_in`, `energy_single` (E after the first single-move descent: quench_device's
    energy_out), `energy_out`, `n_moves` (single moves of all descents), `n_pair_moves`, `n_rounds` (scans), `certified` int32[n_chains];
    and, unless conflicts=False, `conflicts` int16[n_chains][N*N]."""
    n = _device_states("quench_pairs_device", N, states)
    return _device_call(_PAIRS, "quench_pairs_device", (N,), n, states, (max_rounds,), {"conflicts": tuple(states.shape)} if conflicts else {}, out=out, stream=stream)


def quench_pairs(N, states, max_rounds=0, conflicts=True):
    """The pair-move quench of board placements on the GPU: `states` is uint8[n_chains][N*N] (one board of N*N heights is taken as one
    chain), bytes >= N are clamped to N - 1.  The placements descend under single-height moves, then take the best move of two aligned
    columns at once, and so on until a scan finds no improving pair (certified = 1) or, with max_rounds > 0, that many scans have each
    applied a move (certified = 0; the output is still a single-move minimum).  Returns a dict of NumPy arrays with the fields of
    FIELDS_PAIRS; a placement with n_pair_moves == 0 and n_moves == 0 was a 2-move minimum already.  ValueError for what the library
    refuses (N outside 2 .. 32, no chain, a negative max_rounds)."""
    return _round_trip(_PAIRS, (N,), (max_rounds,), _host_states(N, states), lambda: (),
                       lambda t: quench_pairs_device(N, t, max_rounds=max_rounds, conflicts=conflicts))


FIELDS_HOP = ("state", "energy_in", "energy_start", "energy_out", "best_energy", "best_hop", "best_state", "n_accepted", "n_improved", "n_moves",
              "n_pair_moves", "energy_hist")


def _block_hop(N, n, n_hops, kick, slack, local_search, first_hop):
    if local_search not in abi.HOP_LOCAL_SEARCH:
        raise ValueError(f'local_search must be "single" or "pairs", got {local_search!r}')
    q = abi.Hop()
    q.N, q.mode, q.n_chains, q.n_hops, q.first_hop = int(N), abi.MODE_BOARD, int(n), int(n_hops), int(first_hop)
    q.kick, q.slack, q.local_search = int(kick), int(slack), abi.HOP_LOCAL_SEARCH[local_search]
    return q


_HOP = _Search(_block_hop, abi.HOP_DTYPES, _lib.hop_host, _lib.hop_device, ("best_state",), True)


def _hop_seeds(seeds, n):
    s = np.ascontiguousarray(seeds, dtype=np.uint32).reshape(-1)
    if s.shape[0] != n:
        raise ValueError(f"seeds must be uint32[n_chains = {n}], got {s.shape[0]}")
    return s


def hop_host(N, states, seeds, n_hops, kick=2, slack=0, local_search="pairs", first_hop=0, hist=False):
    """mcq_hop_host: basin hopping in the library's plain host code, NumPy in and out, no GPU.  Same result as hop_states."""
    s = _host_states(N, states)
    n, width = s.shape[0], max(int(n_hops), 0) + 1
    return _host_call(_HOP, (N,), s, (n_hops, kick, slack, local_search, first_hop), {"energy_hist": (n, width)} if hist else {}, seeds, width)


def hop_device(N, states, seeds, n_hops, kick=2, slack=0, local_search="pairs", first_hop=0, hist=False, out=None, stream=None):
    """mcq_hop_device on a torch uint8 tensor [n_chains][N*N] of the current device (e.g. DeviceRun.t["best_state"]) and an int32 or
    uint32 tensor `seeds` [n_chains] on the same device (the seeds' 32 bits, whatever the sign), enqueued on `stream` (default: torch's
    current stream).  ONE kernel whatever n_hops is.  Asynchronous: nothing is copied back and nothing synchronises.  `out` (optional)
    is the tensor the final placements go to; it may be `states` itself (in place), default a new one.  Returns a dict of tensors with
    the fields of FIELDS_HOP: `state` and `best_state` uint8 like `states`; `energy_in`, `energy_start`, `energy_out`, `best_energy`
    int32[n_chains]; `best_hop`, `n_accepted`, `n_improved`, `n_moves`, `n_pair_moves` int64[n_chains]; and with hist=True `energy_hist`
    int32[n_chains][n_hops + 1]."""
    n, width = _device_states("hop_device", N, states), max(int(n_hops), 0) + 1
    return _device_call(_HOP, "hop_device", (N,), n, states, (n_hops, kick, slack, local_search, first_hop), {"energy_hist": (n, width)} if hist else {},
                        seeds, width, out=out, stream=stream)


def hop_states(N, states, seeds, n_hops, kick=2, slack=0, local_search="pairs", first_hop=0, hist=False):
    """Basin hopping of board placements on the GPU: `states` is uint8[n_chains][N*N] (one board of N*N heights is taken as one chain),
    bytes >= N are clamped to N - 1; `seeds` is uint32[n_chains].  Every placement first descends to a minimum of the local search --
    "single": single-height moves, "pairs": those and moves of two aligned columns --; then n_hops times `kick` random columns get
    random heights, the local search runs again, and the new minimum stays when its energy is at most the old one + slack; otherwise
    the placement goes back.  Returns a dict of NumPy arrays with the fields of FIELDS_HOP (`energy_hist` only with hist=True).
    A run may be cut: feed `state` back in with first_hop = the hops done so far.  n_accepted, n_moves and n_pair_moves of the pieces add up; best_energy
    / best_state / best_hop of the whole are those of the FIRST piece with the smallest best_energy, its best_hop moved by the hops
    before that piece; n_improved of the whole is the number of new lows of the joined energy_hist (a piece counts against its own
    start, which with slack > 0 may lie above an earlier piece's best_energy).  ValueError for what the library refuses (N outside 2 .. 32, no chain, kick outside 1 .. 1024, a negative
    n_hops, first_hop or slack)."""
    s = _host_states(N, states)
    sd = _hop_seeds(seeds, s.shape[0])
    return _round_trip(_HOP, (N,), (n_hops, kick, slack, local_search, first_hop), s, lambda: (sd.view(np.int32),),
                       lambda t, ts: hop_device(N, t, ts, n_hops, kick=kick, slack=slack, local_search=local_search, first_hop=first_hop, hist=hist))


def check_hops(hops, hop_kick, N, board=True):
    """ValueError for what the competition driver's `hops` hook does not take, before anything is launched."""
    if int(hops) < 0:
        raise ValueError(f"hops must be >= 0, got {hops}")
    if int(hops) == 0:
        return
    if not board:
        raise ValueError('hops: basin hopping runs boards only (mcmc_type="board")')
    if not abi.MIN_N <= int(N) <= abi.MAX_N_QUENCH_PAIRS:
        raise ValueError(f"hops: N out of range [{abi.MIN_N}, {abi.MAX_N_QUENCH_PAIRS}]: {N}")
    if not 1 <= int(hop_kick) <= abi.MAX_HOP_KICK:
        raise ValueError(f"hop_kick out of range [1, {abi.MAX_HOP_KICK}]: {hop_kick}")


FIELDS_TABU = ("state", "energy_in", "energy_out", "best_energy", "best_iter", "best_state", "n_moves", "n_aspired", "n_uphill", "n_stalled",
               "energy_hist", "tabu_out")


def _block_tabu(N, n, n_iters, tenure, tenure_rand, tenure_conf, first_iter):
    q = abi.Tabu()
    q.N, q.mode, q.n_chains, q.n_iters, q.first_iter = int(N), abi.MODE_BOARD, int(n), int(n_iters), int(first_iter)
    q.tenure, q.tenure_rand, q.tenure_conf = int(tenure), int(tenure_rand), int(tenure_conf)
    return q


_TABU = _Search(_block_tabu, abi.TABU_DTYPES, _lib.tabu_host, _lib.tabu_device, ("best_state",), True)


def _tabu_shapes(n, width, cube, hist, tabu_out):
    """The rows a tabu call was asked for: the history and the stamps."""
    return dict({"energy_hist": (n, width)} if hist else {}, **({"tabu_out": (n, cube)} if tabu_out else {}))


def _tabu_host_inputs(n, cube, tabu_in, best_floor):
    """What an earlier piece of a run hands the host entry of a tabu search, as {field: array}; ValueError for another size."""
    ins = {}
    if tabu_in is not None:
        ins["tabu_in"] = np.ascontiguousarray(tabu_in, dtype=np.uint16).reshape(-1)
        if ins["tabu_in"].shape[0] != n * cube:
            raise ValueError(f"tabu_in must be uint16[n_chains = {n}][N^3 = {cube}], got {np.shape(tabu_in)}")
    if best_floor is not None:
        ins["best_floor"] = np.ascontiguousarray(best_floor, dtype=np.int32).reshape(-1)
        if ins["best_floor"].shape[0] != n:
            raise ValueError(f"best_floor must be int32[n_chains = {n}], got {np.shape(best_floor)}")
    return ins


def _tabu_device_inputs(fn, n, cube, dev, tabu_in, best_floor):
    """_tabu_host_inputs for the device wrapper `fn`: the tensors checked, nothing converted."""
    import torch

    if tabu_in is not None and not (isinstance(tabu_in, torch.Tensor) and tabu_in.device == dev and tabu_in.is_contiguous() and tabu_in.numel() == n * cube
                                    and tabu_in.dtype in (torch.int16, getattr(torch, "uint16", torch.int16))):
        raise ValueError(f"{fn} takes tabu_in as a contiguous int16 or uint16 tensor [n_chains = {n}][N^3 = {cube}] on the device of states")
    if best_floor is not None and not (isinstance(best_floor, torch.Tensor) and best_floor.device == dev and best_floor.is_contiguous()
                                       and best_floor.dtype == torch.int32 and tuple(best_floor.shape) == (n,)):
        raise ValueError(f"{fn} takes best_floor as a contiguous int32 tensor [n_chains = {n}] on the device of states")
    return {k: t for k, t in (("tabu_in", tabu_in), ("best_floor", best_floor)) if t is not None}


def _tabu_arrays(sd, tabu_in, best_floor):
    """The host arrays tabu_states and tabu_queens upload behind the placements: the seeds, the stamps and the floor, as the signed types."""
    return (sd.view(np.int32), None if tabu_in is None else np.ascontiguousarray(tabu_in, dtype=np.uint16).view(np.int16),
            None if best_floor is None else np.ascontiguousarray(best_floor, dtype=np.int32))


def tabu_host(N, states, seeds, n_iters, tenure=10, tenure_rand=0, tenure_conf=0, first_iter=0, tabu_in=None, best_floor=None, hist=False,
              tabu_out=False):
    """mcq_tabu_host: tabu search in the library's plain host code, NumPy in and out, no GPU.  Same result as tabu_states."""
    s = _host_states(N, states)
    n, width, cube = s.shape[0], max(int(n_iters), 0) + 1, s.shape[1] * max(int(N), 0)
    return _host_call(_TABU, (N,), s, (n_iters, tenure, tenure_rand, tenure_conf, first_iter), _tabu_shapes(n, width, cube, hist, tabu_out), seeds, width,
                      lambda: _tabu_host_inputs(n, cube, tabu_in, best_floor))


def tabu_device(N, states, seeds, n_iters, tenure=10, tenure_rand=0, tenure_conf=0, first_iter=0, tabu_in=None, best_floor=None, hist=False,
                tabu_out=False, out=None, stream=None):
    """mcq_tabu_device on a torch uint8 tensor [n_chains][N*N] of the current device (e.g. DeviceRun.t["best_state"]) and an int32 or
    uint32 tensor `seeds` [n_chains] on the same device, enqueued on `stream` (default: torch's current stream).  ONE kernel whatever
    n_iters is.  Asynchronous: nothing is copied back and nothing synchronises.  `tabu_in` (optional) is an int16 or uint16 tensor
    [n_chains][N^3] (the 16 bits, whatever the sign) and `best_floor` an int32 tensor [n_chains], both of an earlier call.  `out`
    (optional) is the tensor the final placements go to; it may be `states` itself (in place), default a new one.  Returns a dict of
    tensors with the fields of FIELDS_TABU: `state` and `best_state` uint8 like `states`; `energy_in`, `energy_out`, `best_energy`
    int32[n_chains]; `best_iter`, `n_moves`, `n_aspired`, `n_uphill`, `n_stalled` int64[n_chains]; with hist=True `energy_hist`
    int32[n_chains][n_iters + 1]; with tabu_out=True `tabu_out` int16[n_chains][N^3] (the uint16 stamps; to_numpy views them so)."""
    n, width, cube = _device_states("tabu_device", N, states), max(int(n_iters), 0) + 1, int(states.shape[1]) * max(int(N), 0)
    return _device_call(_TABU, "tabu_device", (N,), n, states, (n_iters, tenure, tenure_rand, tenure_conf, first_iter), _tabu_shapes(n, width, cube, hist, tabu_out),
                        seeds, width, lambda: _tabu_device_inputs("tabu_device", n, cube, states.device, tabu_in, best_floor), out=out, stream=stream)


def tabu_to_numpy(res):
    """The dict tabu_device returned, as NumPy arrays (tabu_out as uint16).  The stream must have passed the call."""
    out = {k: t.cpu().numpy() for k, t in res.items()}
    if "tabu_out" in out:
        out["tabu_out"] = out["tabu_out"].view(np.uint16)
    return out


def tabu_states(N, states, seeds, n_iters, tenure=10, tenure_rand=0, tenure_conf=0, first_iter=0, tabu_in=None, best_floor=None, hist=False,
                tabu_out=False):
    """Tabu search of board placements on the GPU: `states` is uint8[n_chains][N*N] (one board of N*N heights is taken as one chain),
    bytes >= N are clamped to N - 1; `seeds` is uint32[n_chains].  No descent runs first.  Each of the n_iters iterations takes, over the
    columns whose queen is attacked, the single-height move with the smallest energy change -- a rise too; ties by a random rotation --
    that is not tabu, or that leads below the best energy of the run, and the height it left is tabu for `tenure` iterations + a uniform
    draw from 0 .. tenure_rand + tenure_conf / 16 per conflicting column.  Returns a dict of NumPy arrays with the fields of FIELDS_TABU
    (`energy_hist` only with hist=True, `tabu_out` only with tabu_out=True); best_state is the best placement the call saw, the input
    when best_iter = 0.  A run may be cut: feed `state` back in with first_iter = the iterations done so far, tabu_in = the tabu_out and
    best_floor = the best_energy of the piece before; the counters of the pieces add up, and best_state / best_iter of the whole are
    those of the LAST piece with best_iter > 0.  ValueError for what the library refuses (N outside 2 .. 32, no chain, tenure outside
    0 .. 8192, tenure_rand outside 0 .. 4095, tenure_conf outside 0 .. 64, a negative n_iters or first_iter)."""
    s = _host_states(N, states)
    sd = _hop_seeds(seeds, s.shape[0])
    return _round_trip(_TABU, (N,), (n_iters, tenure, tenure_rand, tenure_conf, first_iter), s, lambda: _tabu_arrays(sd, tabu_in, best_floor),
                       lambda t, ts, ti, bf: tabu_device(N, t, ts, n_iters, tenure=tenure, tenure_rand=tenure_rand, tenure_conf=tenure_conf, first_iter=first_iter,
                                                         tabu_in=ti, best_floor=bf, hist=hist, tabu_out=tabu_out))


def check_tabu(tabu_iters, tabu_tenure, hops, N, board=True):
    """ValueError for what the competition driver's `tabu_iters` hook does not take, before anything is launched."""
    if int(tabu_iters) < 0:
        raise ValueError(f"tabu_iters must be >= 0, got {tabu_iters}")
    if int(tabu_iters) == 0:
        return
    if int(hops):
        raise ValueError("tabu_iters and hops: one search behind the runs, not both")
    if not board:
        raise ValueError('tabu_iters: tabu search runs boards only (mcmc_type="board")')
    if not abi.MIN_N <= int(N) <= abi.MAX_N_QUENCH_PAIRS:
        raise ValueError(f"tabu_iters: N out of range [{abi.MIN_N}, {abi.MAX_N_QUENCH_PAIRS}]: {N}")
    if not 0 <= int(tabu_tenure) <= abi.MAX_TABU_TENURE:
        raise ValueError(f"tabu_tenure out of range [0, {abi.MAX_TABU_TENURE}]: {tabu_tenure}")


FIELDS_RELINK = ("state", "path_best_state", "distance_in", "n_steps", "path_best_step", "energy_in", "path_best_energy", "path_max_energy",
                 "energy_out", "n_moves", "n_pair_moves", "energy_hist")


def _block_relink(N, n, max_steps, min_dist, local_search, walk):
    if local_search not in abi.HOP_LOCAL_SEARCH:
        raise ValueError(f'local_search must be "single" or "pairs", got {local_search!r}')
    q = abi.Relink()
    q.N, q.mode, q.n_chains, q.walk = int(N), abi.MODE_BOARD, int(n), int(walk)
    q.max_steps, q.min_dist, q.local_search = int(max_steps), int(min_dist), abi.HOP_LOCAL_SEARCH[local_search]
    return q


def _relink_width(N, max_steps):
    """W + 1 of the rule, item 5: the entries of a chain's history."""
    return (int(max_steps) if int(max_steps) > 0 else max(int(N), 0) ** 2) + 1


_RELINK = _Search(_block_relink, abi.RELINK_DTYPES, _lib.relink_host, _lib.relink_device, ("path_best_state",), True)


def relink_host(N, states, guides, seeds, max_steps=0, min_dist=1, local_search="pairs", walk=0, hist=False, figures=True):
    """mcq_relink_host: path relinking in the library's plain host code, NumPy in and out, no GPU.  Same result as relink_states."""
    s, g = _host_states(N, states), _host_states(N, guides)
    if g.shape != s.shape:
        raise ValueError(f"guides must have the shape of states, {s.shape}, got {g.shape}")
    n, width = s.shape[0], _relink_width(N, max_steps)
    return _host_call(_RELINK, (N,), s, (max_steps, min_dist, local_search, walk), {"energy_hist": (n, width)} if hist else {}, seeds, width,
                      lambda: {"guide_in": g}, figures)


def relink_device(N, states, guides, seeds, max_steps=0, min_dist=1, local_search="pairs", walk=0, hist=False, figures=True, out=None, stream=None):
    """mcq_relink_device on two torch uint8 tensors [n_chains][N*N] of the current device, the placements and their guides, and an int32
    or uint32 tensor `seeds` [n_chains] on the same device, enqueued on `stream` (default: torch's current stream).  ONE kernel whatever
    the distances are.  Asynchronous: nothing is copied back and nothing synchronises.  `out` (optional) is the tensor the final
    placements go to; it may be `states` itself (in place) and may not be `guides`; default a new one.  Returns a dict of tensors with
    the fields of FIELDS_RELINK: `state` and `path_best_state` uint8 like `states`; `distance_in`, `n_steps`, `path_best_step`,
    `energy_in`, `path_best_energy`, `path_max_energy`, `energy_out` int32[n_chains]; `n_moves`, `n_pair_moves` int64[n_chains]; with
    hist=True `energy_hist` int32[n_chains][W + 1], W = max_steps or N^2.  figures=False leaves every optional output but the history
    out: `state` alone."""
    import torch

    n, width = _device_states("relink_device", N, states), _relink_width(N, max_steps)
    if not (isinstance(guides, torch.Tensor) and guides.device == states.device and guides.dtype == torch.uint8 and guides.is_contiguous() and guides.shape == states.shape):
        raise ValueError("relink_device takes guides as a contiguous uint8 tensor of the shape and device of states")
    return _device_call(_RELINK, "relink_device", (N,), n, states, (max_steps, min_dist, local_search, walk), {"energy_hist": (n, width)} if hist else {},
                        seeds, width, lambda: {"guide_in": guides}, figures, out=out, stream=stream)


def relink_states(N, states, guides, seeds, max_steps=0, min_dist=1, local_search="pairs", walk=0, hist=False, figures=True):
    """Path relinking of board placements on the GPU: `states` and `guides` are uint8[n_chains][N*N] (one board of N*N heights is taken
    as one chain), bytes >= N are clamped to N - 1; `seeds` is uint32[n_chains].  Each placement walks towards its guide: a step gives
    one of the columns in which the two differ the guide's height, the column whose change of energy is smallest -- a rise too; ties by
    a random rotation that `walk` and the seed decide --, for max_steps steps or, with 0, all the way.  Of the placements on the way that
    are at least max(1, min_dist) columns from the start and min_dist from the guide, the one with the smallest energy (`path_best_state`,
    the start when there is none) then descends under the local search -- "single": single-height moves, "pairs": those and moves of
    two aligned columns -- to `state`.  Returns a dict of NumPy arrays with the fields of FIELDS_RELINK (`energy_hist` only with
    hist=True: the energies along the walk, whose largest is `path_max_energy`, the barrier when less `energy_in`).  ValueError for what
    the library refuses (N outside 2 .. 32, no chain, max_steps or min_dist outside 0 .. N^2, a negative walk)."""
    s, g = _host_states(N, states), _host_states(N, guides)
    if g.shape != s.shape:
        raise ValueError(f"guides must have the shape of states, {s.shape}, got {g.shape}")
    sd = _hop_seeds(seeds, s.shape[0])
    return _round_trip(_RELINK, (N,), (max_steps, min_dist, local_search, walk), s, lambda: (g, sd.view(np.int32)),
                       lambda t, tg, ts: relink_device(N, t, tg, ts, max_steps=max_steps, min_dist=min_dist, local_search=local_search, walk=walk, hist=hist,
                                                       figures=figures))


N_IMAGES = 16  # the symmetries of the square times the flip of the heights


def _images(N, b):
    """board_images without its checks: b is [n][N][N], a NumPy array or a torch tensor; returns the list of the 16 images."""
    torch_like = not isinstance(b, np.ndarray)
    out = []
    for f in (0, 1):
        x = (N - 1) - b if f else b
        for m in (0, 1):
            y = (x.transpose(1, 2) if torch_like else x.swapaxes(1, 2)) if m else x
            for r in range(4):
                out.append(y.rot90(r, (1, 2)) if torch_like else np.rot90(y, r, axes=(1, 2)))
    return out


def board_images(N, states):
    """The 16 symmetric images of board placements as [16][n][N*N]: `states` is uint8[n][N*N], a NumPy array or a torch tensor (the
    result is of the same kind, on the same device).  Image s = 8 f + 4 m + r of the board B (B[i][j] the height of column (i, j)) is
    rot90^r(T^m(F^f(B))): first, with f = 1, every height k becomes N - 1 - k; then, with m = 1, the board is transposed; then it
    is turned r quarter turns counter-clockwise (numpy.rot90).  Image 0 is the board itself.  All 16 have the energy of the board: a
    symmetry of the square keeps rows, columns, diagonals and distances, and the flip keeps |k - k'|.  ValueError for an entry >= N (a
    height that the rule would clamp has no flip)."""
    N = int(N)
    if not abi.MIN_N <= N <= abi.MAX_N_BOARD:
        raise ValueError(f"N out of range [{abi.MIN_N}, {abi.MAX_N_BOARD}]: {N}")
    if isinstance(states, np.ndarray) or not hasattr(states, "is_cuda"):
        s = _host_states(N, states)
        if s.size and int(s.max()) >= N:
            raise ValueError(f"board_images: an entry of states is >= N = {N}")
        return np.stack(_images(N, s.reshape(-1, N, N))).reshape(N_IMAGES, s.shape[0], N * N)
    import torch

    if states.dtype != torch.uint8 or states.dim() != 2 or int(states.shape[1]) != N * N:
        raise ValueError(f"states must be uint8[n][{N * N}] (final_state layout of a board), got {tuple(states.shape)}")
    if states.numel() and int(states.max()) >= N:
        raise ValueError(f"board_images: an entry of states is >= N = {N}")
    return torch.stack(_images(N, states.reshape(-1, N, N))).reshape(N_IMAGES, states.shape[0], N * N)


def _nearest(N, s, imgs):
    """(image, index, distance) of nearest_image from the stacked images [16][n][N*N] of the guides; s is [n][N*N]."""
    torch_like = not isinstance(s, np.ndarray)
    if torch_like:
        import torch

        dist = (imgs != s.unsqueeze(0)).sum(dim=2)  # [16][n]
        key = (dist * N_IMAGES + torch.arange(N_IMAGES, device=s.device).unsqueeze(1)).min(dim=0).values  # the smallest index of the smallest distance
        idx = key % N_IMAGES
        return imgs[idx, torch.arange(s.shape[0], device=s.device)].contiguous(), idx.to(torch.int32), (key // N_IMAGES).to(torch.int32)
    dist = (imgs != s[None]).sum(axis=2).astype(np.int64)
    key = (dist * N_IMAGES + np.arange(N_IMAGES)[:, None]).min(axis=0)
    idx = key % N_IMAGES
    return np.ascontiguousarray(imgs[idx, np.arange(s.shape[0])]), idx.astype(np.int32), (key // N_IMAGES).astype(np.int32)


def nearest_image(N, states, guides):
    """Of the 16 images of each guide (board_images) the one closest to its state in Hamming distance: returns (the images uint8[n][N*N],
    their indices int32[n] in board_images' numbering, the distances int32[n]); the smallest index on ties.  Two minima that are mirror
    images of one another are N^2 columns apart and relink through noise; aligned, the walk is as short as the symmetry allows, and the
    guide's energy is the same.  NumPy arrays or torch tensors, both of the same kind; ValueError for an entry >= N in either."""
    imgs = board_images(N, guides)
    if isinstance(imgs, np.ndarray):
        s = _host_states(N, states)
        if s.shape != imgs.shape[1:]:
            raise ValueError(f"states must have the shape of guides, {imgs.shape[1:]}, got {s.shape}")
        if s.size and int(s.max()) >= int(N):
            raise ValueError(f"nearest_image: an entry of states is >= N = {int(N)}")
        return _nearest(int(N), s, imgs)
    if not hasattr(states, "is_cuda") or states.dtype != imgs.dtype or states.device != imgs.device or tuple(states.shape) != tuple(imgs.shape[1:]):
        raise ValueError("nearest_image takes states as a uint8 tensor of the shape and device of guides")
    if states.numel() and int(states.max()) >= int(N):
        raise ValueError(f"nearest_image: an entry of states is >= N = {int(N)}")
    return _nearest(int(N), states, imgs)


def _pool_args(N, n, rounds, min_dist, partner_seed):
    """(min_dist, the shifts s_k of the rounds) of relink_pool / relink_pool_host, and their refusals."""
    if int(rounds) < 1:
        raise ValueError(f"rounds must be >= 1, got {rounds}")
    if n < 2:
        raise ValueError(f"relink_pool needs a pool of at least 2 placements, got {n}")
    N = int(N)
    md = max(1, N * N // 8) if min_dist is None else int(min_dist)
    rs = np.random.RandomState(int(partner_seed))
    return md, [int(rs.randint(1, n)) for _ in range(int(rounds))]


def relink_pool_host(N, states, seeds, rounds, min_dist=None, local_search="pairs", align=True, partner_seed=0):
    """relink_pool in NumPy over relink_host: the same pool, energies and counts, no GPU."""
    s = _host_states(N, states)
    n = s.shape[0]
    md, shifts = _pool_args(N, n, rounds, min_dist, partner_seed)
    if abi.MIN_N <= int(N) <= abi.MAX_N_QUENCH_PAIRS:
        s = np.minimum(s, np.uint8(int(N) - 1))
    sd = _hop_seeds(seeds, n)
    pool, energy, n_replaced, best = s.copy(), None, [], []
    for k, shift in enumerate(shifts):
        guides = np.roll(pool, shift, axis=0)
        if align:
            guides = _nearest(int(N), pool, np.stack(_images(int(N), guides.reshape(-1, int(N), int(N)))).reshape(N_IMAGES, n, -1))[0]
        r = relink_host(N, pool, guides, sd, min_dist=md, local_search=local_search, walk=k)
        better = r["energy_out"] < r["energy_in"]
        pool = np.where(better[:, None], r["state"], pool)
        energy = np.where(better, r["energy_out"], r["energy_in"]).astype(np.int32)
        n_replaced.append(int(better.sum()))
        best.append(int(energy.min()))
    return {"state": pool, "energy": energy, "n_replaced": np.array(n_replaced, dtype=np.int64), "best_energy": np.array(best, dtype=np.int32)}


def relink_pool(N, states, seeds, rounds, min_dist=None, local_search="pairs", align=True, partner_seed=0, stream=None):
    """Rounds of path relinking over a pool of board placements on the GPU: `states` is a torch uint8 tensor [n][N*N] on the device
    (n >= 2; bytes >= N are clamped to N - 1 first), `seeds` an int32 or uint32 tensor [n].  Round k = 0 .. rounds - 1 takes as the
    guide of slot r the placement of slot (r - s_k) mod n (torch.roll by s_k, drawn from 1 .. n - 1 with
    np.random.RandomState(partner_seed), one draw per round), with align=True its image closest to the slot's placement (nearest_image),
    and calls relink_device with walk = k and min_dist (default max(1, N^2 / 8)).  A slot takes the call's `state` when its energy_out
    is strictly below the slot's own energy; otherwise it keeps its placement.  Everything stays on the device, on `stream` (default:
    torch's current stream), with one synchronisation at the end.  Returns a dict: `state` uint8[n][N*N] and `energy` int32[n], tensors;
    `n_replaced` int64[rounds] and `best_energy` int32[rounds] (the pool's smallest energy behind each round), NumPy arrays."""
    import torch

    n = _device_states("relink_pool", N, states)
    md, shifts = _pool_args(N, n, rounds, min_dist, partner_seed)
    N = int(N)
    dev = states.device
    st = torch.cuda.current_stream(dev) if stream is None else stream
    with torch.cuda.device(dev), torch.cuda.stream(st):
        pool = states.clamp(max=N - 1) if abi.MIN_N <= N <= abi.MAX_N_QUENCH_PAIRS else states
        energy, n_replaced, best = None, [], []
        for k, shift in enumerate(shifts):
            guides = torch.roll(pool, shift, 0)
            if align:
                guides = _nearest(N, pool, torch.stack(_images(N, guides.reshape(-1, N, N))).reshape(N_IMAGES, n, -1))[0]
            r = relink_device(N, pool, guides, seeds, min_dist=md, local_search=local_search, walk=k, stream=st)
            better = r["energy_out"] < r["energy_in"]
            pool = torch.where(better.unsqueeze(1), r["state"], pool)
            energy = torch.where(better, r["energy_out"], r["energy_in"])
            n_replaced.append(better.sum())
            best.append(energy.min())
        n_replaced, best = torch.stack(n_replaced), torch.stack(best)
        st.synchronize()
    return {"state": pool, "energy": energy, "n_replaced": n_replaced.cpu().numpy().astype(np.int64), "best_energy": best.cpu().numpy().astype(np.int32)}


def check_mode(quench, N, board=True):
    """ValueError for a `quench` the annealing hooks do not take: the one string they know is "pairs", which runs boards up to
    N = abi.MAX_N_QUENCH_PAIRS only.  Anything else is read as a truth value, as before."""
    if not isinstance(quench, str):
        return
    if quench != "pairs":
        raise ValueError(f'quench must be False, True or "pairs", got {quench!r}')
    if not board:
        raise ValueError('quench="pairs": the pair-move quench runs boards only (mcmc_type="board")')
    if not abi.MIN_N <= int(N) <= abi.MAX_N_QUENCH_PAIRS:
        raise ValueError(f'quench="pairs": N out of range [{abi.MIN_N}, {abi.MAX_N_QUENCH_PAIRS}]: {N}')


def hook_device(N, best_state, quench, stream):
    """What an annealing hook enqueues behind its last fold on a board's best_state: quench_device, or quench_pairs_device for "pairs"."""
    if quench == "pairs":
        return quench_pairs_device(N, best_state, conflicts=False, stream=stream)
    return quench_device(N, best_state, conflicts=False, stream=stream)


def hook_results(res, quenched):
    """The hook's fields in a result dict: quenched_state, quenched_energy, quench_moves, and behind "pairs" also quench_pair_moves,
    quench_rounds, quench_certified and quench_energy_single."""
    res["quenched_state"], res["quenched_energy"] = quenched["state"].cpu().numpy(), quenched["energy_out"].cpu().numpy()
    res["quench_moves"] = quenched["n_moves"].cpu().numpy()
    if "n_pair_moves" in quenched:
        res["quench_pair_moves"], res["quench_rounds"] = quenched["n_pair_moves"].cpu().numpy(), quenched["n_rounds"].cpu().numpy()
        res["quench_certified"], res["quench_energy_single"] = quenched["certified"].cpu().numpy(), quenched["energy_single"].cpu().numpy()


FIELDS_3D = ("state", "energy_in", "energy_out", "n_moves", "n_passes", "conflicts", "flags")


def _block3d(N, Q, n, max_passes):
    q = abi.Quench3D()
    q.N, q.n_queens, q.n_chains, q.max_passes = int(N), int(Q), int(n), int(max_passes)
    return q


_QUENCH3D = _Search(_block3d, abi.QUENCH3D_DTYPES, _lib.quench3d_host, _lib.quench3d_device, (), False)


def _queens_of(N, Q):
    return int(N) * int(N) if Q is None or int(Q) == 0 else int(Q)


def _host_queens(N, states, Q):
    """uint8[n][3 Q] from uint8[n][3 Q] or [n][Q][3] (one placement [Q][3] or [3 Q] is taken as one chain)."""
    s = np.ascontiguousarray(states, dtype=np.uint8)
    Q = _queens_of(N, Q)
    if s.size == 0:
        return s.reshape(0, 3 * max(Q, 0))
    if s.ndim == 1 or (s.ndim == 2 and s.shape == (Q, 3)):  # one placement
        s = s.reshape(1, -1)
    s = s.reshape(s.shape[0], -1)
    if abi.MIN_N <= int(N) <= abi.MAX_N_QUENCH3D and Q >= 2 and s.shape[1] != 3 * Q:
        raise ValueError(f"states must be uint8[n_chains][{3 * Q}] or [n_chains][{Q}][3] (final_state layout of full_3d), got {s.shape}")
    return s


def quench_queens_host(N, states, Q=None, max_passes=0, conflicts=True):
    """mcq_quench3d_host: the full_3d rule in the library's plain host code, NumPy in and out, no GPU.  Same result as quench_queens."""
    s, Qn = _host_queens(N, states, Q), _queens_of(N, Q)
    return _host_call(_QUENCH3D, (N, Qn), s, (max_passes,), {"conflicts": (s.shape[0], s.shape[1] // 3)} if conflicts else {})


def quench_queens_device(N, states, Q=None, max_passes=0, out=None, conflicts=True, stream=None):
    """mcq_quench3d_device on a torch uint8 tensor [n_chains][3 Q] or [n_chains][Q][3] of the current device (e.g.
    DeviceRun.t["best_state"] of a full_3d run), enqueued on `stream` (default: torch's current stream).  Asynchronous: nothing is copied
    back and nothing synchronises, so the results are valid once the stream has passed the call.  `out` (optional) is the tensor the
    placements go to; it may be `states` itself (in place), default a new one.  Returns a dict of tensors: `state` uint8 like `states`,
    `energy_in` (the recount of the input), `energy_out`, `n_moves`, `n_passes`, `flags` int32[n_chains] and, unless conflicts=False,
    `conflicts` int16[n_chains][Q] (the uint16 counts a(q, pos(q)) of the output; below 2^15, so the sign bit is never set)."""
    n, Qn = _device_queens("quench_queens_device", N, states, Q)
    return _device_call(_QUENCH3D, "quench_queens_device", (N, Qn), n, states, (max_passes,), {"conflicts": (n, Qn)} if conflicts else {}, out=out, stream=stream)


def quench_queens(N, states, Q=None, max_passes=0, conflicts=True):
    """Quench full_3d placements on the GPU: `states` is uint8[n_chains][3 Q] or [n_chains][Q][3] (the final_state / best_state layout
    of a full_3d run: Q triples (i, j, k); Q=None means N^2), bytes >= N are clamped to N - 1.  max_passes = 0 runs until a pass moves
    nothing.  Returns a dict of NumPy arrays: `state` uint8[n_chains][3 Q] (the placements after the descent), `energy_in` (the energy
    of the input, recounted on the device), `energy_out`, `n_moves`, `n_passes`, `flags` int32[n_chains], and `conflicts`
    uint16[n_chains][Q], the number of queens attacking each queen in the output (its sum is 2 energy_out).  A placement with
    n_moves == 0 and n_passes == 1 was a local minimum already; flags bit 0 (abi.QUENCH3D_REPEATED) marks an input with two queens in
    one cell, which is recounted and handed back unmoved.  ValueError for what the library refuses (N outside 2 .. 32, Q outside
    2 .. N^3 - 1, no chain, a negative max_passes)."""
    return _round_trip(_QUENCH3D, (N, _queens_of(N, Q)), (max_passes,), _host_queens(N, states, Q), lambda: (),
                       lambda t: quench_queens_device(N, t, Q=Q, max_passes=max_passes, conflicts=conflicts))


FIELDS_HOP3D = ("state", "energy_in", "energy_start", "energy_out", "best_energy", "best_hop", "best_state", "n_accepted", "n_improved", "n_moves",
                "n_passes", "n_kicked", "energy_hist", "flags")


def _block_hop3d(N, Q, n, n_hops, kick, slack, first_hop):
    q = abi.Hop3d()
    q.N, q.n_queens, q.n_chains, q.n_hops, q.first_hop = int(N), int(Q), int(n), int(n_hops), int(first_hop)
    q.kick, q.slack = int(kick), int(slack)
    return q


_HOP3D = _Search(_block_hop3d, abi.HOP3D_DTYPES, _lib.hop3d_host, _lib.hop3d_device, ("best_state",), True)


def hop_queens_host(N, states, seeds, n_hops, Q=None, kick=2, slack=0, first_hop=0, hist=False):
    """mcq_hop3d_host: basin hopping of full_3d placements in the library's plain host code, NumPy in and out, no GPU.  Same result as
    hop_queens, and it runs every shape (the kernel stops where a chain no longer fits the LDS: abi.hop3d_lds_bytes)."""
    s = _host_queens(N, states, Q)
    n, width = s.shape[0], max(int(n_hops), 0) + 1
    return _host_call(_HOP3D, (N, _queens_of(N, Q)), s, (n_hops, kick, slack, first_hop), {"energy_hist": (n, width)} if hist else {}, seeds, width)


def hop_queens_device(N, states, seeds, n_hops, Q=None, kick=2, slack=0, first_hop=0, hist=False, out=None, stream=None):
    """mcq_hop3d_device on a torch uint8 tensor [n_chains][3 Q] or [n_chains][Q][3] of the current device (e.g. DeviceRun.t["best_state"]
    of a full_3d run; Q=None means N^2) and an int32 or uint32 tensor `seeds` [n_chains] on the same device (the seeds' 32 bits, whatever
    the sign), enqueued on `stream` (default: torch's current stream).  ONE kernel whatever n_hops is.  Asynchronous: nothing is copied
    back and nothing synchronises.  `out` (optional) is the tensor the final placements go to; it may be `states` itself (in place),
    default a new one.  Returns a dict of tensors with the fields of FIELDS_HOP3D: `state` and `best_state` uint8 like `states`;
    `energy_in`, `energy_start`, `energy_out`, `best_energy`, `flags` int32[n_chains]; `best_hop`, `n_accepted`, `n_improved`, `n_moves`,
    `n_passes`, `n_kicked` int64[n_chains]; and with hist=True `energy_hist` int32[n_chains][n_hops + 1]."""
    (n, Qn), width = _device_queens("hop_queens_device", N, states, Q), max(int(n_hops), 0) + 1
    return _device_call(_HOP3D, "hop_queens_device", (N, Qn), n, states, (n_hops, kick, slack, first_hop), {"energy_hist": (n, width)} if hist else {},
                        seeds, width, out=out, stream=stream)


def hop_queens(N, states, seeds, n_hops, Q=None, kick=2, slack=0, first_hop=0, hist=False):
    """Basin hopping of full_3d placements on the GPU: `states` is uint8[n_chains][3 Q] or [n_chains][Q][3] (Q triples (i, j, k); Q=None
    means N^2), bytes >= N are clamped to N - 1; `seeds` is uint32[n_chains].  Every placement first descends to a minimum under
    single-queen moves (quench_queens with max_passes = 0); then n_hops times `kick` random queens are drawn with a random cell each and
    move there when it is free, the descent runs again, and the new minimum stays when its energy is at most the old one + slack;
    otherwise the placement goes back.  Returns a dict of NumPy arrays with the fields of FIELDS_HOP3D, `state` and `best_state`
    uint8[n_chains][3 Q] (`energy_hist` only with hist=True); flags bit 0 (abi.HOP3D_REPEATED) marks an input with two queens in one
    cell, which is recounted and handed back unmoved.  A run may be cut: feed `state` back in with first_hop = the hops done so far; the
    figures of the pieces combine as hop_states says, n_passes in the place of n_pair_moves.  ValueError for what the library refuses
    (N outside 2 .. 32, Q outside 2 .. N^3 - 1, no chain, kick outside 1 .. 1024, a negative n_hops, first_hop or slack, a chain above
    the LDS of a workgroup: N = 32 runs up to Q = 23 520)."""
    s = _host_queens(N, states, Q)
    sd = _hop_seeds(seeds, s.shape[0])
    return _round_trip(_HOP3D, (N, _queens_of(N, Q)), (n_hops, kick, slack, first_hop), s, lambda: (sd.view(np.int32),),
                       lambda t, ts: hop_queens_device(N, t, ts, n_hops, Q=Q, kick=kick, slack=slack, first_hop=first_hop, hist=hist))


FIELDS_TABU3D = FIELDS_TABU + ("flags",)


def _block_tabu3d(N, Q, n, n_iters, tenure, tenure_rand, tenure_conf, first_iter):
    q = abi.Tabu3d()
    q.N, q.n_queens, q.n_chains, q.n_iters, q.first_iter = int(N), int(Q), int(n), int(n_iters), int(first_iter)
    q.tenure, q.tenure_rand, q.tenure_conf = int(tenure), int(tenure_rand), int(tenure_conf)
    return q


_TABU3D = _Search(_block_tabu3d, abi.TABU3D_DTYPES, _lib.tabu3d_host, _lib.tabu3d_device, ("best_state",), True)


def tabu_queens_host(N, states, seeds, n_iters, Q=None, tenure=10, tenure_rand=0, tenure_conf=0, first_iter=0, tabu_in=None, best_floor=None,
                     hist=False, tabu_out=False):
    """mcq_tabu3d_host: tabu search of full_3d placements in the library's plain host code, NumPy in and out, no GPU.  Same result as
    tabu_queens, and it runs every shape (the kernel stops where a chain no longer fits the LDS: abi.tabu3d_lds_bytes)."""
    s = _host_queens(N, states, Q)
    n, width, cube = s.shape[0], max(int(n_iters), 0) + 1, max(int(N), 0) ** 3
    return _host_call(_TABU3D, (N, _queens_of(N, Q)), s, (n_iters, tenure, tenure_rand, tenure_conf, first_iter), _tabu_shapes(n, width, cube, hist, tabu_out),
                      seeds, width, lambda: _tabu_host_inputs(n, cube, tabu_in, best_floor))


def tabu_queens_device(N, states, seeds, n_iters, Q=None, tenure=10, tenure_rand=0, tenure_conf=0, first_iter=0, tabu_in=None, best_floor=None,
                       hist=False, tabu_out=False, out=None, stream=None):
    """mcq_tabu3d_device on a torch uint8 tensor [n_chains][3 Q] or [n_chains][Q][3] of the current device (e.g. DeviceRun.t["best_state"]
    of a full_3d run; Q=None means N^2) and an int32 or uint32 tensor `seeds` [n_chains] on the same device, enqueued on `stream`
    (default: torch's current stream).  ONE kernel whatever n_iters is.  Asynchronous: nothing is copied back and nothing synchronises.
    `tabu_in` (optional) is an int16 or uint16 tensor [n_chains][N^3] (the 16 bits, whatever the sign) and `best_floor` an int32 tensor
    [n_chains], both of an earlier call.  `out` (optional) is the tensor the final placements go to; it may be `states` itself (in
    place), default a new one.  Returns a dict of tensors with the fields of FIELDS_TABU3D: `state` and `best_state` uint8 like
    `states`; `energy_in`, `energy_out`, `best_energy`, `flags` int32[n_chains]; `best_iter`, `n_moves`, `n_aspired`, `n_uphill`,
    `n_stalled` int64[n_chains]; with hist=True `energy_hist` int32[n_chains][n_iters + 1]; with tabu_out=True `tabu_out`
    int16[n_chains][N^3] (the uint16 stamps; tabu_to_numpy views them so)."""
    (n, Qn), width, cube = _device_queens("tabu_queens_device", N, states, Q), max(int(n_iters), 0) + 1, max(int(N), 0) ** 3
    return _device_call(_TABU3D, "tabu_queens_device", (N, Qn), n, states, (n_iters, tenure, tenure_rand, tenure_conf, first_iter),
                        _tabu_shapes(n, width, cube, hist, tabu_out), seeds, width,
                        lambda: _tabu_device_inputs("tabu_queens_device", n, cube, states.device, tabu_in, best_floor), out=out, stream=stream)


def tabu_queens(N, states, seeds, n_iters, Q=None, tenure=10, tenure_rand=0, tenure_conf=0, first_iter=0, tabu_in=None, best_floor=None,
                hist=False, tabu_out=False):
    """Tabu search of full_3d placements on the GPU: `states` is uint8[n_chains][3 Q] or [n_chains][Q][3] (Q triples (i, j, k); Q=None
    means N^2), bytes >= N are clamped to N - 1; `seeds` is uint32[n_chains].  No descent runs first.  Each of the n_iters iterations
    takes, over the queens that are attacked and the free cells of the cube, the move with the smallest energy change -- a rise too;
    ties by a random rotation of the queens and of the cells -- whose cell is not tabu, or that leads below the best energy of the run,
    and the cell it left is tabu for `tenure` iterations + a uniform draw from 0 .. tenure_rand + tenure_conf / 16 per conflicting queen
    (at most abi.MAX_TABU3D_SPAN in all).  Returns a dict of NumPy arrays with the fields of FIELDS_TABU3D (`energy_hist` only with
    hist=True, `tabu_out` only with tabu_out=True); best_state is the best placement the call saw, the input when best_iter = 0; flags
    bit 0 (abi.TABU3D_REPEATED) marks an input with two queens in one cell, which is recounted and handed back unmoved.  A run may be
    cut as tabu_states says.  A shape whose chain is above the LDS of a workgroup (abi.tabu3d_lds_bytes(N, Q) > abi.MAX_TABU3D_LDS:
    N = 32 runs up to Q = 14 272 on the device) is run by tabu_queens_host, which gives the same result.  ValueError for what the
    library refuses (N outside 2 .. 32, Q outside 2 .. N^3 - 1, no chain, tenure outside 0 .. 8192, tenure_rand outside 0 .. 4095,
    tenure_conf outside 0 .. 64, a negative n_iters or first_iter)."""
    s = _host_queens(N, states, Q)
    sd = _hop_seeds(seeds, s.shape[0])
    kw = dict(Q=Q, tenure=tenure, tenure_rand=tenure_rand, tenure_conf=tenure_conf, first_iter=first_iter, hist=hist, tabu_out=tabu_out)
    # (no chain is refused by _round_trip, as before the fallback: the host wrapper would look at tabu_in first)
    if s.shape[0] and abi.MIN_N <= int(N) <= abi.MAX_N_QUENCH3D and abi.tabu3d_lds_bytes(N, Q) > abi.MAX_TABU3D_LDS:
        return tabu_queens_host(N, s, sd, n_iters, tabu_in=tabu_in, best_floor=best_floor, **kw)
    return _round_trip(_TABU3D, (N, _queens_of(N, Q)), (n_iters, tenure, tenure_rand, tenure_conf, first_iter), s, lambda: _tabu_arrays(sd, tabu_in, best_floor),
                       lambda t, ts, ti, bf: tabu_queens_device(N, t, ts, n_iters, tabu_in=ti, best_floor=bf, **kw))


def check_tabu_queens(tabu_iters, tabu_tenure, tabu_tenure_rand, hops, N, Q, board):
    """ValueError for what the full_3d annealing hook's `tabu_iters` does not take, before anything is launched."""
    if int(tabu_iters) < 0:
        raise ValueError(f"tabu_iters must be >= 0, got {tabu_iters}")
    if int(tabu_iters) == 0:
        return
    if int(hops):
        raise ValueError("tabu_iters and hops: one search behind the run, not both")
    if board:
        raise ValueError('tabu_iters: this hook runs full_3d placements only (mcmc_type="full_3d"); boards go through quench.tabu_states')
    if not 0 <= int(tabu_tenure) <= abi.MAX_TABU_TENURE:
        raise ValueError(f"tabu_tenure out of range [0, {abi.MAX_TABU_TENURE}]: {tabu_tenure}")
    if not 0 <= int(tabu_tenure_rand) <= abi.MAX_TABU_TENURE_RAND:
        raise ValueError(f"tabu_tenure_rand out of range [0, {abi.MAX_TABU_TENURE_RAND}]: {tabu_tenure_rand}")
    if abi.MIN_N <= int(N) <= abi.MAX_N_QUENCH3D and abi.tabu3d_lds_bytes(N, Q) > abi.MAX_TABU3D_LDS:
        raise ValueError(f"tabu_iters: N = {N} with Q = {_queens_of(N, Q)} takes {abi.tabu3d_lds_bytes(N, Q)} bytes of LDS, above the "
                         f"{abi.MAX_TABU3D_LDS} of a workgroup")


def queens_of_boards(N, boards):
    """Board placements as full_3d placements: heights uint8[n][N*N] (one board is taken as one chain; bytes >= N are clamped to N - 1)
    -> the triples (i, j, h(i, j)) in row-major order of the columns, uint8[n][3 N^2].  The energy of the result in the cube is the
    board's: two queens of different columns attack each other in the cube exactly when the board rule says so.  It carries board minima
    into hop_queens, where the queens may leave their columns."""
    N = int(N)
    h = np.minimum(_host_states(N, boards), N - 1).astype(np.uint8)
    out = np.empty((h.shape[0], N * N, 3), dtype=np.uint8)
    c = np.arange(N * N)
    out[:, :, 0], out[:, :, 1], out[:, :, 2] = (c // N).astype(np.uint8), (c % N).astype(np.uint8), h
    return out.reshape(h.shape[0], 3 * N * N)


FIELDS_RELINK3D = ("state", "path_best_state", "distance_in", "n_steps", "path_best_step", "energy_in", "path_best_energy", "path_max_energy",
                   "energy_out", "n_moves", "n_passes", "energy_hist", "flags")


def _block_relink3d(N, Q, n, max_steps, min_dist, walk):
    q = abi.Relink3d()
    q.N, q.n_queens, q.n_chains, q.walk = int(N), int(Q), int(n), int(walk)
    q.max_steps, q.min_dist = int(max_steps), int(min_dist)
    return q


def _relink3d_width(N, Q, max_steps):
    """W + 1 of the rule, item 5: the entries of a chain's history."""
    return (int(max_steps) if int(max_steps) > 0 else max(_queens_of(N, Q), 0)) + 1


_RELINK3D = _Search(_block_relink3d, abi.RELINK3D_DTYPES, _lib.relink3d_host, _lib.relink3d_device, ("path_best_state",), True)


def relink_queens_host(N, states, guides, seeds, Q=None, max_steps=0, min_dist=1, walk=0, hist=False, figures=True):
    """mcq_relink3d_host: path relinking of full_3d placements in the library's plain host code, NumPy in and out, no GPU.  Same result
    as relink_queens, and it runs every shape (the kernel stops where a chain no longer fits the LDS: abi.relink3d_lds_bytes)."""
    s, g = _host_queens(N, states, Q), _host_queens(N, guides, Q)
    if g.shape != s.shape:
        raise ValueError(f"guides must have the shape of states, {s.shape}, got {g.shape}")
    n, width = s.shape[0], _relink3d_width(N, Q, max_steps)
    return _host_call(_RELINK3D, (N, _queens_of(N, Q)), s, (max_steps, min_dist, walk), {"energy_hist": (n, width)} if hist else {}, seeds, width,
                      lambda: {"guide_in": g}, figures)


def relink_queens_device(N, states, guides, seeds, Q=None, max_steps=0, min_dist=1, walk=0, hist=False, figures=True, out=None, stream=None):
    """mcq_relink3d_device on two torch uint8 tensors [n_chains][3 Q] or [n_chains][Q][3] of the current device, the placements and
    their guides (Q=None means N^2), and an int32 or uint32 tensor `seeds` [n_chains] on the same device, enqueued on `stream` (default:
    torch's current stream).  ONE kernel whatever the distances are.  Asynchronous: nothing is copied back and nothing synchronises.
    `out` (optional) is the tensor the final placements go to; it may be `states` itself (in place) and may not be `guides`; default a
    new one.  Returns a dict of tensors with the fields of FIELDS_RELINK3D: `state` and `path_best_state` uint8 like `states`;
    `distance_in`, `n_steps`, `path_best_step`, `energy_in`, `path_best_energy`, `path_max_energy`, `energy_out`, `flags`
    int32[n_chains]; `n_moves`, `n_passes` int64[n_chains]; with hist=True `energy_hist` int32[n_chains][W + 1], W = max_steps or Q.
    figures=False leaves every optional output but the history out: `state` alone."""
    import torch

    (n, Qn), width = _device_queens("relink_queens_device", N, states, Q), _relink3d_width(N, Q, max_steps)
    if not (isinstance(guides, torch.Tensor) and guides.device == states.device and guides.dtype == torch.uint8 and guides.is_contiguous() and guides.shape == states.shape):
        raise ValueError("relink_queens_device takes guides as a contiguous uint8 tensor of the shape and device of states")
    return _device_call(_RELINK3D, "relink_queens_device", (N, Qn), n, states, (max_steps, min_dist, walk), {"energy_hist": (n, width)} if hist else {},
                        seeds, width, lambda: {"guide_in": guides}, figures, out=out, stream=stream)


def relink_queens(N, states, guides, seeds, Q=None, max_steps=0, min_dist=1, walk=0, hist=False, figures=True):
    """Path relinking of full_3d placements on the GPU: `states` and `guides` are uint8[n_chains][3 Q] or [n_chains][Q][3] (Q triples
    (i, j, k); Q=None means N^2), bytes >= N are clamped to N - 1; `seeds` is uint32[n_chains].  A guide is read as a SET of cells: the
    order of its queens means nothing.  Each placement walks towards its guide: a step moves one of the queens that stand on no cell of
    the guide to one of the guide's cells that hold no queen, the (queen, cell) pair whose change of energy is smallest -- a rise too;
    ties by a random rotation of the queens and of the cells that `walk` and the seed decide --, for max_steps steps or, with 0, all the
    way.  Of the placements on the way that are at least max(1, min_dist) moves from the start and min_dist from the guide, the one with
    the smallest energy (`path_best_state`, the start when there is none) then descends under single-queen moves (quench_queens with
    max_passes = 0) to `state`; queens keep the indices they have in `states`.  Returns a dict of NumPy arrays with the fields of
    FIELDS_RELINK3D (`energy_hist` only with hist=True); flags bit 0 (abi.RELINK3D_REPEATED) marks a placement and bit 1
    (abi.RELINK3D_GUIDE_REPEATED) a guide with two queens in one cell: the chain is recounted and handed back unmoved.  A shape whose
    chain is above the LDS of a workgroup (abi.relink3d_lds_bytes(N, Q) > abi.MAX_RELINK3D_LDS: N = 32 runs up to Q = 11 248 on the
    device) is run by relink_queens_host, which gives the same result.  ValueError for what the library refuses (N outside 2 .. 32, Q
    outside 2 .. N^3 - 1, no chain, max_steps or min_dist outside 0 .. Q, a negative walk)."""
    s, g = _host_queens(N, states, Q), _host_queens(N, guides, Q)
    if g.shape != s.shape:
        raise ValueError(f"guides must have the shape of states, {s.shape}, got {g.shape}")
    sd = _hop_seeds(seeds, s.shape[0])
    kw = dict(Q=Q, max_steps=max_steps, min_dist=min_dist, walk=walk, hist=hist, figures=figures)
    if s.shape[0] and abi.MIN_N <= int(N) <= abi.MAX_N_QUENCH3D and abi.relink3d_lds_bytes(N, Q) > abi.MAX_RELINK3D_LDS:
        return relink_queens_host(N, s, g, sd, **kw)
    return _round_trip(_RELINK3D, (N, _queens_of(N, Q)), (max_steps, min_dist, walk), s, lambda: (g, sd.view(np.int32)),
                       lambda t, tg, ts: relink_queens_device(N, t, tg, ts, **kw))


N_QUEENS_IMAGES = 48  # the symmetries of the cube: the 6 orders of the axes times the 8 mirrorings
_AXES = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))


def _queens_image(N, t, s):
    """Image s of the triples t, [n][Q][3] (NumPy or torch), without checks."""
    perm, flips = _AXES[s >> 3], ((s >> 2) & 1, (s >> 1) & 1, s & 1)
    cols = [(N - 1) - t[..., perm[a]] if flips[a] else t[..., perm[a]] for a in range(3)]
    if isinstance(t, np.ndarray):
        return np.stack(cols, axis=-1)
    import torch

    return torch.stack(cols, dim=-1)


def _queens_triples(fn, N, states, Q):
    """The triples [n][Q][3] of queens_images / nearest_queens_image, NumPy or torch, with their checks."""
    N, Qn = int(N), _queens_of(N, Q)
    if not abi.MIN_N <= N <= abi.MAX_N_QUENCH3D:
        raise ValueError(f"N out of range [{abi.MIN_N}, {abi.MAX_N_QUENCH3D}]: {N}")
    if isinstance(states, np.ndarray) or not hasattr(states, "is_cuda"):
        t = _host_queens(N, states, Q)
    else:
        import torch

        ok = (states.dim() == 2 and int(states.shape[1]) == 3 * Qn) or (states.dim() == 3 and tuple(states.shape[1:]) == (Qn, 3))
        if states.dtype != torch.uint8 or not ok:
            raise ValueError(f"states must be uint8[n][{3 * Qn}] or [n][{Qn}][3] (final_state layout of full_3d), got {tuple(states.shape)}")
        t = states
    t = t.reshape(t.shape[0], Qn, 3)
    if t.shape[0] and Qn and int(t.max()) >= N:
        raise ValueError(f"{fn}: an entry of states is >= N = {N}")
    return t


def queens_images(N, states, Q=None):
    """The 48 images of full_3d placements under the symmetries of the cube, as [48][n][3 Q]: `states` is uint8[n][3 Q] or [n][Q][3], a
    NumPy array or a torch tensor (the result is of the same kind, on the same device; Q=None means N^2).  Image s = 8 p + 4 f0 + 2 f1 +
    f2 of a queen x = (x0, x1, x2): first the axes are reordered, y_a = x_{P[p][a]} with P = ((0, 1, 2), (0, 2, 1), (1, 0, 2),
    (1, 2, 0), (2, 0, 1), (2, 1, 0)) (itertools.permutations order); then, where f_a = 1, y_a becomes N - 1 - y_a.  Image 0 is the
    placement itself; queens keep their indices.  All 48 have the energy of the placement: a reordering of the axes and a mirroring
    keep |di|, |dj|, |dk| as a set, which is all the attack rule reads.  ValueError for an entry >= N (a byte that the rule would clamp
    has no mirror image)."""
    t = _queens_triples("queens_images", N, states, Q)
    imgs = [_queens_image(int(N), t, s).reshape(t.shape[0], -1) for s in range(N_QUEENS_IMAGES)]
    if isinstance(t, np.ndarray):
        return np.stack(imgs)
    import torch

    return torch.stack(imgs)


def _cell_sets(N, t):
    """The cells of the triples t, [n][Q][3], as a bitmap bool[n][N^3] (NumPy or torch)."""
    n, C = t.shape[0], N ** 3
    if isinstance(t, np.ndarray):
        cell = (t[..., 0].astype(np.int64) * N + t[..., 1]) * N + t[..., 2]
        occ = np.zeros((n, C), dtype=bool)
        occ[np.arange(n)[:, None], cell] = True
        return occ
    import torch

    cell = (t[..., 0].to(torch.int64) * N + t[..., 1]) * N + t[..., 2]
    return torch.zeros((n, C), dtype=torch.bool, device=t.device).scatter_(1, cell, True)


def _nearest_queens(N, ts, tg):
    """(image, index, distance) of nearest_queens_image from checked triples [n][Q][3] of one kind."""
    occ = _cell_sets(N, ts)
    best = None
    for s in range(N_QUEENS_IMAGES):  # ascending, and replaced only when strictly nearer: the smallest index on ties
        img = _queens_image(N, tg, s)
        dist = (occ & ~_cell_sets(N, img)).sum(1)
        if best is None:
            best = [img, dist * 0 + s, dist]
            continue
        nearer = dist < best[2]
        if isinstance(ts, np.ndarray):
            best = [np.where(nearer[:, None, None], img, best[0]), np.where(nearer, s, best[1]), np.where(nearer, dist, best[2])]
        else:
            import torch

            best = [torch.where(nearer[:, None, None], img, best[0]), torch.where(nearer, s, best[1]), torch.where(nearer, dist, best[2])]
    img = best[0].reshape(ts.shape[0], -1)
    if isinstance(ts, np.ndarray):
        return np.ascontiguousarray(img), best[1].astype(np.int32), best[2].astype(np.int32)
    import torch

    return img.contiguous(), best[1].to(torch.int32), best[2].to(torch.int32)


def nearest_queens_image(N, states, guides, Q=None):
    """Of the 48 images of each guide (queens_images) the one with the smallest set distance |cells(A) \\ cells(G')| to its placement A:
    returns (the images uint8[n][3 Q], their indices int32[n] in queens_images' numbering, the distances int32[n]); the smallest index
    on ties.  The distance is the d0 of relink_queens between the two, so an aligned walk is as short as the cube's symmetry allows,
    and the guide's energy is the same.  NumPy arrays or torch tensors, both of the same kind; no kernel of the library runs.
    ValueError for an entry >= N in either."""
    tg = _queens_triples("nearest_queens_image", N, guides, Q)
    if isinstance(tg, np.ndarray) != (isinstance(states, np.ndarray) or not hasattr(states, "is_cuda")):
        raise ValueError("nearest_queens_image takes states and guides of the same kind, NumPy arrays or torch tensors")
    ts = _queens_triples("nearest_queens_image", N, states, Q)
    if tuple(ts.shape) != tuple(tg.shape) or (not isinstance(tg, np.ndarray) and ts.device != tg.device):
        raise ValueError(f"states must have the shape and device of guides, {tuple(tg.shape)}, got {tuple(ts.shape)}")
    return _nearest_queens(int(N), ts, tg)


def _queens_pool_args(N, Q, n, rounds, min_dist, partner_seed):
    """(min_dist, the shifts s_k of the rounds) of relink_queens_pool / relink_queens_pool_host, and their refusals."""
    if int(rounds) < 1:
        raise ValueError(f"rounds must be >= 1, got {rounds}")
    if n < 2:
        raise ValueError(f"relink_queens_pool needs a pool of at least 2 placements, got {n}")
    md = max(1, _queens_of(N, Q) // 8) if min_dist is None else int(min_dist)
    rs = np.random.RandomState(int(partner_seed))
    return md, [int(rs.randint(1, n)) for _ in range(int(rounds))]


def relink_queens_pool_host(N, states, seeds, rounds, Q=None, min_dist=None, align=True, partner_seed=0):
    """relink_queens_pool in NumPy over relink_queens_host: the same pool, energies and counts, no GPU."""
    s = _host_queens(N, states, Q)
    n = s.shape[0]
    md, shifts = _queens_pool_args(N, Q, n, rounds, min_dist, partner_seed)
    if abi.MIN_N <= int(N) <= abi.MAX_N_QUENCH3D:
        s = np.minimum(s, np.uint8(int(N) - 1))
    sd = _hop_seeds(seeds, n)
    pool, energy, n_replaced, best = s.copy(), None, [], []
    for k, shift in enumerate(shifts):
        guides = np.roll(pool, shift, axis=0)
        if align:
            guides = _nearest_queens(int(N), pool.reshape(n, -1, 3), guides.reshape(n, -1, 3))[0]
        r = relink_queens_host(N, pool, guides, sd, Q=Q, min_dist=md, walk=k)
        better = r["energy_out"] < r["energy_in"]
        pool = np.where(better[:, None], r["state"], pool)
        energy = np.where(better, r["energy_out"], r["energy_in"]).astype(np.int32)
        n_replaced.append(int(better.sum()))
        best.append(int(energy.min()))
    return {"state": pool, "energy": energy, "n_replaced": np.array(n_replaced, dtype=np.int64), "best_energy": np.array(best, dtype=np.int32)}


def relink_queens_pool(N, states, seeds, rounds, Q=None, min_dist=None, align=True, partner_seed=0, stream=None):
    """Rounds of path relinking over a pool of full_3d placements on the GPU: `states` is a torch uint8 tensor [n][3 Q] on the device
    (n >= 2; bytes >= N are clamped to N - 1 first; Q=None means N^2), `seeds` an int32 or uint32 tensor [n].  Round k = 0 .. rounds - 1
    takes as the guide of slot r the placement of slot (r - s_k) mod n (torch.roll by s_k, drawn from 1 .. n - 1 with
    np.random.RandomState(partner_seed), one draw per round), with align=True its image closest to the slot's placement
    (nearest_queens_image), and calls relink_queens_device with walk = k and min_dist (default max(1, Q / 8)).  A slot takes the call's
    `state` when its energy_out is strictly below the slot's own energy; otherwise it keeps its placement.  Everything stays on the
    device, on `stream` (default: torch's current stream), with one synchronisation at the end.  Returns a dict: `state` uint8[n][3 Q]
    and `energy` int32[n], tensors; `n_replaced` int64[rounds] and `best_energy` int32[rounds] (the pool's smallest energy behind each
    round), NumPy arrays."""
    import torch

    n, Qn = _device_queens("relink_queens_pool", N, states, Q)
    if states.dim() != 2:
        raise ValueError(f"relink_queens_pool takes states as uint8[n][{3 * Qn}], got {tuple(states.shape)}")
    md, shifts = _queens_pool_args(N, Q, n, rounds, min_dist, partner_seed)
    N = int(N)
    dev = states.device
    st = torch.cuda.current_stream(dev) if stream is None else stream
    with torch.cuda.device(dev), torch.cuda.stream(st):
        pool = states.clamp(max=N - 1) if abi.MIN_N <= N <= abi.MAX_N_QUENCH3D else states
        energy, n_replaced, best = None, [], []
        for k, shift in enumerate(shifts):
            guides = torch.roll(pool, shift, 0)
            if align:
                guides = _nearest_queens(N, pool.reshape(n, -1, 3), guides.reshape(n, -1, 3))[0]
            r = relink_queens_device(N, pool, guides, seeds, Q=Q, min_dist=md, walk=k, stream=st)
            better = r["energy_out"] < r["energy_in"]
            pool = torch.where(better.unsqueeze(1), r["state"], pool)
            energy = torch.where(better, r["energy_out"], r["energy_in"])
            n_replaced.append(better.sum())
            best.append(energy.min())
        n_replaced, best = torch.stack(n_replaced), torch.stack(best)
        st.synchronize()
    return {"state": pool, "energy": energy, "n_replaced": n_replaced.cpu().numpy().astype(np.int64), "best_energy": best.cpu().numpy().astype(np.int32)}
