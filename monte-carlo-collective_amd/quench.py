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
"""
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


def _device_outputs(q, states, out, dtypes, conflicts):
    """The result tensors of a quench on the device, from a *_DTYPES table -- int32 per chain, and `conflicts` int16 of the shape given
    (None: left out) --, with the block `q` pointed at them and at `states`.  `out` is _device_out's."""
    import torch

    res = {"state": _device_out(out, states)}
    for k in dtypes:
        if k != "conflicts":
            res[k] = torch.empty(int(states.shape[0]), dtype=torch.int32, device=states.device)
        elif conflicts is not None:
            res[k] = torch.empty(conflicts, dtype=torch.int16, device=states.device)
    q.state_in, q.state_out = states.data_ptr(), res["state"].data_ptr()
    for k in dtypes:
        if k in res:
            setattr(q, k, res[k].data_ptr())
    return res


def quench_states_host(N, states, max_passes=0, conflicts=True):
    """mcq_quench_host: the rule in the library's plain host code, NumPy in and out, no GPU.  Same result as quench_states."""
    s = _host_states(N, states)
    q = _block(N, s.shape[0], max_passes)
    out = _host_outputs(q, s, abi.QUENCH_DTYPES, {"conflicts": s.shape}, () if conflicts else ("conflicts",))
    _lib.quench_host(q)
    return out


def quench_device(N, states, max_passes=0, out=None, conflicts=True, stream=None):
    """mcq_quench_device on a torch uint8 tensor [n_chains][N*N] of the current device (e.g. DeviceRun.t["best_state"]), enqueued on
    `stream` (default: torch's current stream).  Asynchronous: nothing is copied back and nothing synchronises, so the results are valid
    once the stream has passed the call.  `out` (optional) is the tensor the placements go to; it may be `states` itself (in place),
    default a new one.  Returns a dict of tensors: `state` uint8 like `states`, `energy_in` (the recount of the input), `energy_out`,
    `n_moves`, `n_passes` int32[n_chains] and, unless conflicts=False, `conflicts` int16[n_chains][N*N] (the uint16 counts a(c, h(c)) of the
    output; at most 4 (N - 1), so the sign bit is never set)."""
    import torch

    n = _device_states("quench_device", N, states)
    dev = states.device
    st = torch.cuda.current_stream(dev) if stream is None else stream
    with torch.cuda.device(dev), torch.cuda.stream(st):
        q = _block(N, n, max_passes)
        res = _device_outputs(q, states, out, abi.QUENCH_DTYPES, tuple(states.shape) if conflicts else None)
        _lib.quench_device(q, st)
    return res


def quench_states(N, states, max_passes=0, conflicts=True):
    """Quench board placements on the GPU: `states` is uint8[n_chains][N*N] (the final_state / best_state layout; one board of N*N
    heights is taken as one chain), bytes >= N are clamped to N - 1.  max_passes = 0 runs until a pass makes no move.  Returns a dict of
    NumPy arrays: `state` (the placements after the descent), `energy_in` (the energy of the input, recounted on the device),
    `energy_out`, `n_moves`, `n_passes` int32[n_chains], and `conflicts` uint16[n_chains][N*N], the number of queens attacking each
    column's queen in the output (its sum is 2 energy_out).  A placement with n_moves == 0 was a local minimum already.
    ValueError for what the library refuses (N outside 2 .. 128, no chain, a negative max_passes)."""
    import torch

    s = _host_states(N, states)
    if s.shape[0] == 0:
        _lib.quench_host(_block(N, 0, max_passes))  # raises the library's refusal
    dev = torch.device("cuda", torch.cuda.current_device())
    res = quench_device(N, torch.from_numpy(s).to(dev), max_passes=max_passes, conflicts=conflicts)
    torch.cuda.current_stream(dev).synchronize()
    return to_numpy(res)


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


def quench_pairs_host(N, states, max_rounds=0, conflicts=True):
    """mcq_quench_pairs_host: the pair-move rule in the library's plain host code, NumPy in and out, no GPU.  Same result as
    quench_pairs."""
    s = _host_states(N, states)
    q = _block_pairs(N, s.shape[0], max_rounds)
    out = _host_outputs(q, s, abi.QUENCH_PAIRS_DTYPES, {"conflicts": s.shape}, () if conflicts else ("conflicts",))
    _lib.quench_pairs_host(q)
    return out


def quench_pairs_device(N, states, max_rounds=0, out=None, conflicts=True, stream=None):
    """mcq_quench_pairs_device on a torch uint8 tensor [n_chains][N*N] of the current device (e.g. DeviceRun.t["best_state"]), enqueued
    on `stream` (default: torch's current stream).  Asynchronous like quench_device: nothing is copied back and nothing synchronises.
    `out` (optional) is the tensor the placements go to; it may be `states` itself (in place), default a new one.  Returns a dict of
    tensors: `state` uint8 like `states`; `energy_in`, `energy_single` (E after the first single-move descent: quench_device's
    energy_out), `energy_out`, `n_moves` (single moves of all descents), `n_pair_moves`, `n_rounds` (scans), `certified` int32[n_chains];
    and, unless conflicts=False, `conflicts` int16[n_chains][N*N]."""
    import torch

    n = _device_states("quench_pairs_device", N, states)
    dev = states.device
    st = torch.cuda.current_stream(dev) if stream is None else stream
    with torch.cuda.device(dev), torch.cuda.stream(st):
        q = _block_pairs(N, n, max_rounds)
        res = _device_outputs(q, states, out, abi.QUENCH_PAIRS_DTYPES, tuple(states.shape) if conflicts else None)
        _lib.quench_pairs_device(q, st)
    return res


def quench_pairs(N, states, max_rounds=0, conflicts=True):
    """The pair-move quench of board placements on the GPU: `states` is uint8[n_chains][N*N] (one board of N*N heights is taken as one
    chain), bytes >= N are clamped to N - 1.  The placements descend under single-height moves, then take the best move of two aligned
    columns at once, and so on until a scan finds no improving pair (certified = 1) or, with max_rounds > 0, that many scans have each
    applied a move (certified = 0; the output is still a single-move minimum).  Returns a dict of NumPy arrays with the fields of
    FIELDS_PAIRS; a placement with n_pair_moves == 0 and n_moves == 0 was a 2-move minimum already.  ValueError for what the library
    refuses (N outside 2 .. 32, no chain, a negative max_rounds)."""
    import torch

    s = _host_states(N, states)
    if s.shape[0] == 0:
        _lib.quench_pairs_host(_block_pairs(N, 0, max_rounds))  # raises the library's refusal
    dev = torch.device("cuda", torch.cuda.current_device())
    res = quench_pairs_device(N, torch.from_numpy(s).to(dev), max_rounds=max_rounds, conflicts=conflicts)
    torch.cuda.current_stream(dev).synchronize()
    return to_numpy(res)


FIELDS_HOP = ("state", "energy_in", "energy_start", "energy_out", "best_energy", "best_hop", "best_state", "n_accepted", "n_improved", "n_moves",
              "n_pair_moves", "energy_hist")


def _block_hop(N, n, n_hops, kick, slack, local_search, first_hop):
    if local_search not in abi.HOP_LOCAL_SEARCH:
        raise ValueError(f'local_search must be "single" or "pairs", got {local_search!r}')
    q = abi.Hop()
    q.N, q.mode, q.n_chains, q.n_hops, q.first_hop = int(N), abi.MODE_BOARD, int(n), int(n_hops), int(first_hop)
    q.kick, q.slack, q.local_search = int(kick), int(slack), abi.HOP_LOCAL_SEARCH[local_search]
    return q


def _hop_seeds(seeds, n):
    s = np.ascontiguousarray(seeds, dtype=np.uint32).reshape(-1)
    if s.shape[0] != n:
        raise ValueError(f"seeds must be uint32[n_chains = {n}], got {s.shape[0]}")
    return s


def hop_host(N, states, seeds, n_hops, kick=2, slack=0, local_search="pairs", first_hop=0, hist=False):
    """mcq_hop_host: basin hopping in the library's plain host code, NumPy in and out, no GPU.  Same result as hop_states."""
    s = _host_states(N, states)
    n = s.shape[0]
    sd = _hop_seeds(seeds, n)
    q = _block_hop(N, n, n_hops, kick, slack, local_search, first_hop)
    width = max(int(n_hops), 0) + 1
    out = _host_outputs(q, s, abi.HOP_DTYPES, {"energy_hist": (n, width)}, () if hist else ("energy_hist",), like=("best_state",))
    q.seeds, q.hist_stride = sd.ctypes.data, width
    _lib.hop_host(q)
    return out


def hop_device(N, states, seeds, n_hops, kick=2, slack=0, local_search="pairs", first_hop=0, hist=False, out=None, stream=None):
    """mcq_hop_device on a torch uint8 tensor [n_chains][N*N] of the current device (e.g. DeviceRun.t["best_state"]) and an int32 or
    uint32 tensor `seeds` [n_chains] on the same device (the seeds' 32 bits, whatever the sign), enqueued on `stream` (default: torch's
    current stream).  ONE kernel whatever n_hops is.  Asynchronous: nothing is copied back and nothing synchronises.  `out` (optional)
    is the tensor the final placements go to; it may be `states` itself (in place), default a new one.  Returns a dict of tensors with
    the fields of FIELDS_HOP: `state` and `best_state` uint8 like `states`; `energy_in`, `energy_start`, `energy_out`, `best_energy`
    int32[n_chains]; `best_hop`, `n_accepted`, `n_improved`, `n_moves`, `n_pair_moves` int64[n_chains]; and with hist=True `energy_hist`
    int32[n_chains][n_hops + 1]."""
    import torch

    n = _device_states("hop_device", N, states)
    dev = states.device
    if not (isinstance(seeds, torch.Tensor) and seeds.device == dev and seeds.dtype in (torch.int32, getattr(torch, "uint32", torch.int32)) and seeds.is_contiguous()
            and tuple(seeds.shape) == (n,)):
        raise ValueError(f"hop_device takes seeds as a contiguous int32 or uint32 tensor [n_chains = {n}] on the device of states")
    st = torch.cuda.current_stream(dev) if stream is None else stream
    with torch.cuda.device(dev), torch.cuda.stream(st):
        q = _block_hop(N, n, n_hops, kick, slack, local_search, first_hop)
        width = max(int(n_hops), 0) + 1
        res = {"state": _device_out(out, states), "best_state": torch.empty_like(states)}
        for k, dt in abi.HOP_DTYPES.items():
            if k != "energy_hist":
                res[k] = torch.empty(n, dtype=torch.int64 if dt is np.int64 else torch.int32, device=dev)
            elif hist:
                res[k] = torch.empty((n, width), dtype=torch.int32, device=dev)
        q.seeds, q.state_in, q.state_out, q.best_state, q.hist_stride = seeds.data_ptr(), states.data_ptr(), res["state"].data_ptr(), res["best_state"].data_ptr(), width
        for k in abi.HOP_DTYPES:
            if k in res:
                setattr(q, k, res[k].data_ptr())
        _lib.hop_device(q, st)
    return res


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
    import torch

    s = _host_states(N, states)
    sd = _hop_seeds(seeds, s.shape[0])
    if s.shape[0] == 0:
        _lib.hop_host(_block_hop(N, 0, n_hops, kick, slack, local_search, first_hop))  # raises the library's refusal
    dev = torch.device("cuda", torch.cuda.current_device())
    res = hop_device(N, torch.from_numpy(s).to(dev), torch.from_numpy(sd.view(np.int32)).to(dev), n_hops, kick=kick, slack=slack,
                     local_search=local_search, first_hop=first_hop, hist=hist)
    torch.cuda.current_stream(dev).synchronize()
    return to_numpy(res)


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


def _tabu_skip(hist, tabu_out):
    return (() if hist else ("energy_hist",)) + (() if tabu_out else ("tabu_out",))


def tabu_host(N, states, seeds, n_iters, tenure=10, tenure_rand=0, tenure_conf=0, first_iter=0, tabu_in=None, best_floor=None, hist=False,
              tabu_out=False):
    """mcq_tabu_host: tabu search in the library's plain host code, NumPy in and out, no GPU.  Same result as tabu_states."""
    s = _host_states(N, states)
    n = s.shape[0]
    sd = _hop_seeds(seeds, n)
    q = _block_tabu(N, n, n_iters, tenure, tenure_rand, tenure_conf, first_iter)
    width, cube = max(int(n_iters), 0) + 1, s.shape[1] * max(int(N), 0)
    out = _host_outputs(q, s, abi.TABU_DTYPES, {"energy_hist": (n, width), "tabu_out": (n, cube)}, _tabu_skip(hist, tabu_out), like=("best_state",))
    q.seeds, q.hist_stride = sd.ctypes.data, width
    keep = []
    if tabu_in is not None:
        keep.append(np.ascontiguousarray(tabu_in, dtype=np.uint16).reshape(-1))
        if keep[-1].shape[0] != n * cube:
            raise ValueError(f"tabu_in must be uint16[n_chains = {n}][N^3 = {cube}], got {np.shape(tabu_in)}")
        q.tabu_in = keep[-1].ctypes.data
    if best_floor is not None:
        keep.append(np.ascontiguousarray(best_floor, dtype=np.int32).reshape(-1))
        if keep[-1].shape[0] != n:
            raise ValueError(f"best_floor must be int32[n_chains = {n}], got {np.shape(best_floor)}")
        q.best_floor = keep[-1].ctypes.data
    _lib.tabu_host(q)
    return out


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
    import torch

    n = _device_states("tabu_device", N, states)
    dev = states.device
    if not (isinstance(seeds, torch.Tensor) and seeds.device == dev and seeds.dtype in (torch.int32, getattr(torch, "uint32", torch.int32)) and seeds.is_contiguous()
            and tuple(seeds.shape) == (n,)):
        raise ValueError(f"tabu_device takes seeds as a contiguous int32 or uint32 tensor [n_chains = {n}] on the device of states")
    cube = int(states.shape[1]) * max(int(N), 0)
    if tabu_in is not None and not (isinstance(tabu_in, torch.Tensor) and tabu_in.device == dev and tabu_in.is_contiguous() and tabu_in.numel() == n * cube
                                    and tabu_in.dtype in (torch.int16, getattr(torch, "uint16", torch.int16))):
        raise ValueError(f"tabu_device takes tabu_in as a contiguous int16 or uint16 tensor [n_chains = {n}][N^3 = {cube}] on the device of states")
    if best_floor is not None and not (isinstance(best_floor, torch.Tensor) and best_floor.device == dev and best_floor.is_contiguous()
                                       and best_floor.dtype == torch.int32 and tuple(best_floor.shape) == (n,)):
        raise ValueError(f"tabu_device takes best_floor as a contiguous int32 tensor [n_chains = {n}] on the device of states")
    st = torch.cuda.current_stream(dev) if stream is None else stream
    with torch.cuda.device(dev), torch.cuda.stream(st):
        q = _block_tabu(N, n, n_iters, tenure, tenure_rand, tenure_conf, first_iter)
        width = max(int(n_iters), 0) + 1
        res = {"state": _device_out(out, states), "best_state": torch.empty_like(states)}
        for k, dt in abi.TABU_DTYPES.items():
            if k == "energy_hist":
                if hist:
                    res[k] = torch.empty((n, width), dtype=torch.int32, device=dev)
            elif k == "tabu_out":
                if tabu_out:
                    res[k] = torch.empty((n, cube), dtype=torch.int16, device=dev)
            else:
                res[k] = torch.empty(n, dtype=torch.int64 if dt is np.int64 else torch.int32, device=dev)
        q.seeds, q.state_in, q.state_out, q.best_state, q.hist_stride = seeds.data_ptr(), states.data_ptr(), res["state"].data_ptr(), res["best_state"].data_ptr(), width
        if tabu_in is not None:
            q.tabu_in = tabu_in.data_ptr()
        if best_floor is not None:
            q.best_floor = best_floor.data_ptr()
        for k in abi.TABU_DTYPES:
            if k in res:
                setattr(q, k, res[k].data_ptr())
        _lib.tabu_device(q, st)
    return res


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
    import torch

    s = _host_states(N, states)
    sd = _hop_seeds(seeds, s.shape[0])
    if s.shape[0] == 0:
        _lib.tabu_host(_block_tabu(N, 0, n_iters, tenure, tenure_rand, tenure_conf, first_iter))  # raises the library's refusal
    dev = torch.device("cuda", torch.cuda.current_device())
    ti = None if tabu_in is None else torch.from_numpy(np.ascontiguousarray(tabu_in, dtype=np.uint16).view(np.int16)).to(dev)
    bf = None if best_floor is None else torch.from_numpy(np.ascontiguousarray(best_floor, dtype=np.int32)).to(dev)
    res = tabu_device(N, torch.from_numpy(s).to(dev), torch.from_numpy(sd.view(np.int32)).to(dev), n_iters, tenure=tenure, tenure_rand=tenure_rand,
                      tenure_conf=tenure_conf, first_iter=first_iter, tabu_in=ti, best_floor=bf, hist=hist, tabu_out=tabu_out)
    torch.cuda.current_stream(dev).synchronize()
    return tabu_to_numpy(res)


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


def _relink_skip(hist, figures):
    return tuple(k for k in abi.RELINK_DTYPES if (k == "energy_hist" and not hist) or (k != "energy_hist" and not figures))


def relink_host(N, states, guides, seeds, max_steps=0, min_dist=1, local_search="pairs", walk=0, hist=False, figures=True):
    """mcq_relink_host: path relinking in the library's plain host code, NumPy in and out, no GPU.  Same result as relink_states."""
    s, g = _host_states(N, states), _host_states(N, guides)
    n = s.shape[0]
    if g.shape != s.shape:
        raise ValueError(f"guides must have the shape of states, {s.shape}, got {g.shape}")
    sd = _hop_seeds(seeds, n)
    q = _block_relink(N, n, max_steps, min_dist, local_search, walk)
    width = _relink_width(N, max_steps)
    out = _host_outputs(q, s, abi.RELINK_DTYPES, {"energy_hist": (n, width)}, _relink_skip(hist, figures), like=("path_best_state",) if figures else ())
    q.seeds, q.guide_in, q.hist_stride = sd.ctypes.data, g.ctypes.data, width
    _lib.relink_host(q)
    return out


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

    n = _device_states("relink_device", N, states)
    dev = states.device
    if not (isinstance(guides, torch.Tensor) and guides.device == dev and guides.dtype == torch.uint8 and guides.is_contiguous() and guides.shape == states.shape):
        raise ValueError("relink_device takes guides as a contiguous uint8 tensor of the shape and device of states")
    if not (isinstance(seeds, torch.Tensor) and seeds.device == dev and seeds.dtype in (torch.int32, getattr(torch, "uint32", torch.int32)) and seeds.is_contiguous()
            and tuple(seeds.shape) == (n,)):
        raise ValueError(f"relink_device takes seeds as a contiguous int32 or uint32 tensor [n_chains = {n}] on the device of states")
    st = torch.cuda.current_stream(dev) if stream is None else stream
    with torch.cuda.device(dev), torch.cuda.stream(st):
        q = _block_relink(N, n, max_steps, min_dist, local_search, walk)
        width = _relink_width(N, max_steps)
        res = {"state": _device_out(out, states)}
        if figures:
            res["path_best_state"] = torch.empty_like(states)
            q.path_best_state = res["path_best_state"].data_ptr()
        for k, dt in abi.RELINK_DTYPES.items():
            if k == "energy_hist":
                if hist:
                    res[k] = torch.empty((n, width), dtype=torch.int32, device=dev)
            elif figures:
                res[k] = torch.empty(n, dtype=torch.int64 if dt is np.int64 else torch.int32, device=dev)
        q.seeds, q.state_in, q.guide_in, q.state_out, q.hist_stride = seeds.data_ptr(), states.data_ptr(), guides.data_ptr(), res["state"].data_ptr(), width
        for k in abi.RELINK_DTYPES:
            if k in res:
                setattr(q, k, res[k].data_ptr())
        _lib.relink_device(q, st)
    return res


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
    import torch

    s, g = _host_states(N, states), _host_states(N, guides)
    if g.shape != s.shape:
        raise ValueError(f"guides must have the shape of states, {s.shape}, got {g.shape}")
    sd = _hop_seeds(seeds, s.shape[0])
    if s.shape[0] == 0:
        _lib.relink_host(_block_relink(N, 0, max_steps, min_dist, local_search, walk))  # raises the library's refusal
    dev = torch.device("cuda", torch.cuda.current_device())
    res = relink_device(N, torch.from_numpy(s).to(dev), torch.from_numpy(g).to(dev), torch.from_numpy(sd.view(np.int32)).to(dev), max_steps=max_steps,
                        min_dist=min_dist, local_search=local_search, walk=walk, hist=hist, figures=figures)
    torch.cuda.current_stream(dev).synchronize()
    return to_numpy(res)


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
    s = _host_queens(N, states, Q)
    n = s.shape[0]
    q = _block3d(N, _queens_of(N, Q), n, max_passes)
    out = _host_outputs(q, s, abi.QUENCH3D_DTYPES, {"conflicts": (n, s.shape[1] // 3)}, () if conflicts else ("conflicts",))
    _lib.quench3d_host(q)
    return out


def quench_queens_device(N, states, Q=None, max_passes=0, out=None, conflicts=True, stream=None):
    """mcq_quench3d_device on a torch uint8 tensor [n_chains][3 Q] or [n_chains][Q][3] of the current device (e.g.
    DeviceRun.t["best_state"] of a full_3d run), enqueued on `stream` (default: torch's current stream).  Asynchronous: nothing is copied
    back and nothing synchronises, so the results are valid once the stream has passed the call.  `out` (optional) is the tensor the
    placements go to; it may be `states` itself (in place), default a new one.  Returns a dict of tensors: `state` uint8 like `states`,
    `energy_in` (the recount of the input), `energy_out`, `n_moves`, `n_passes`, `flags` int32[n_chains] and, unless conflicts=False,
    `conflicts` int16[n_chains][Q] (the uint16 counts a(q, pos(q)) of the output; below 2^15, so the sign bit is never set)."""
    import torch

    n, Qn = _device_queens("quench_queens_device", N, states, Q)
    dev = states.device
    st = torch.cuda.current_stream(dev) if stream is None else stream
    with torch.cuda.device(dev), torch.cuda.stream(st):
        q = _block3d(N, Qn, n, max_passes)
        res = _device_outputs(q, states, out, abi.QUENCH3D_DTYPES, (n, Qn) if conflicts else None)
        _lib.quench3d_device(q, st)
    return res


def quench_queens(N, states, Q=None, max_passes=0, conflicts=True):
    """Quench full_3d placements on the GPU: `states` is uint8[n_chains][3 Q] or [n_chains][Q][3] (the final_state / best_state layout
    of a full_3d run: Q triples (i, j, k); Q=None means N^2), bytes >= N are clamped to N - 1.  max_passes = 0 runs until a pass moves
    nothing.  Returns a dict of NumPy arrays: `state` uint8[n_chains][3 Q] (the placements after the descent), `energy_in` (the energy
    of the input, recounted on the device), `energy_out`, `n_moves`, `n_passes`, `flags` int32[n_chains], and `conflicts`
    uint16[n_chains][Q], the number of queens attacking each queen in the output (its sum is 2 energy_out).  A placement with
    n_moves == 0 and n_passes == 1 was a local minimum already; flags bit 0 (abi.QUENCH3D_REPEATED) marks an input with two queens in
    one cell, which is recounted and handed back unmoved.  ValueError for what the library refuses (N outside 2 .. 32, Q outside
    2 .. N^3 - 1, no chain, a negative max_passes)."""
    import torch

    s = _host_queens(N, states, Q)
    if s.shape[0] == 0:
        _lib.quench3d_host(_block3d(N, _queens_of(N, Q), 0, max_passes))  # raises the library's refusal
    dev = torch.device("cuda", torch.cuda.current_device())
    res = quench_queens_device(N, torch.from_numpy(s).to(dev), Q=Q, max_passes=max_passes, conflicts=conflicts)
    torch.cuda.current_stream(dev).synchronize()
    return to_numpy(res)


FIELDS_HOP3D = ("state", "energy_in", "energy_start", "energy_out", "best_energy", "best_hop", "best_state", "n_accepted", "n_improved", "n_moves",
                "n_passes", "n_kicked", "energy_hist", "flags")


def _block_hop3d(N, Q, n, n_hops, kick, slack, first_hop):
    q = abi.Hop3d()
    q.N, q.n_queens, q.n_chains, q.n_hops, q.first_hop = int(N), int(Q), int(n), int(n_hops), int(first_hop)
    q.kick, q.slack = int(kick), int(slack)
    return q


def hop_queens_host(N, states, seeds, n_hops, Q=None, kick=2, slack=0, first_hop=0, hist=False):
    """mcq_hop3d_host: basin hopping of full_3d placements in the library's plain host code, NumPy in and out, no GPU.  Same result as
    hop_queens, and it runs every shape (the kernel stops where a chain no longer fits the LDS: abi.hop3d_lds_bytes)."""
    s = _host_queens(N, states, Q)
    n = s.shape[0]
    sd = _hop_seeds(seeds, n)
    q = _block_hop3d(N, _queens_of(N, Q), n, n_hops, kick, slack, first_hop)
    width = max(int(n_hops), 0) + 1
    out = _host_outputs(q, s, abi.HOP3D_DTYPES, {"energy_hist": (n, width)}, () if hist else ("energy_hist",), like=("best_state",))
    q.seeds, q.hist_stride = sd.ctypes.data, width
    _lib.hop3d_host(q)
    return out


def hop_queens_device(N, states, seeds, n_hops, Q=None, kick=2, slack=0, first_hop=0, hist=False, out=None, stream=None):
    """mcq_hop3d_device on a torch uint8 tensor [n_chains][3 Q] or [n_chains][Q][3] of the current device (e.g. DeviceRun.t["best_state"]
    of a full_3d run; Q=None means N^2) and an int32 or uint32 tensor `seeds` [n_chains] on the same device (the seeds' 32 bits, whatever
    the sign), enqueued on `stream` (default: torch's current stream).  ONE kernel whatever n_hops is.  Asynchronous: nothing is copied
    back and nothing synchronises.  `out` (optional) is the tensor the final placements go to; it may be `states` itself (in place),
    default a new one.  Returns a dict of tensors with the fields of FIELDS_HOP3D: `state` and `best_state` uint8 like `states`;
    `energy_in`, `energy_start`, `energy_out`, `best_energy`, `flags` int32[n_chains]; `best_hop`, `n_accepted`, `n_improved`, `n_moves`,
    `n_passes`, `n_kicked` int64[n_chains]; and with hist=True `energy_hist` int32[n_chains][n_hops + 1]."""
    import torch

    n, Qn = _device_queens("hop_queens_device", N, states, Q)
    dev = states.device
    if not (isinstance(seeds, torch.Tensor) and seeds.device == dev and seeds.dtype in (torch.int32, getattr(torch, "uint32", torch.int32)) and seeds.is_contiguous()
            and tuple(seeds.shape) == (n,)):
        raise ValueError(f"hop_queens_device takes seeds as a contiguous int32 or uint32 tensor [n_chains = {n}] on the device of states")
    st = torch.cuda.current_stream(dev) if stream is None else stream
    with torch.cuda.device(dev), torch.cuda.stream(st):
        q = _block_hop3d(N, Qn, n, n_hops, kick, slack, first_hop)
        width = max(int(n_hops), 0) + 1
        res = {"state": _device_out(out, states), "best_state": torch.empty_like(states)}
        for k, dt in abi.HOP3D_DTYPES.items():
            if k != "energy_hist":
                res[k] = torch.empty(n, dtype=torch.int64 if dt is np.int64 else torch.int32, device=dev)
            elif hist:
                res[k] = torch.empty((n, width), dtype=torch.int32, device=dev)
        q.seeds, q.state_in, q.state_out, q.best_state, q.hist_stride = seeds.data_ptr(), states.data_ptr(), res["state"].data_ptr(), res["best_state"].data_ptr(), width
        for k in abi.HOP3D_DTYPES:
            if k in res:
                setattr(q, k, res[k].data_ptr())
        _lib.hop3d_device(q, st)
    return res


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
    import torch

    s = _host_queens(N, states, Q)
    sd = _hop_seeds(seeds, s.shape[0])
    if s.shape[0] == 0:
        _lib.hop3d_host(_block_hop3d(N, _queens_of(N, Q), 0, n_hops, kick, slack, first_hop))  # raises the library's refusal
    dev = torch.device("cuda", torch.cuda.current_device())
    res = hop_queens_device(N, torch.from_numpy(s).to(dev), torch.from_numpy(sd.view(np.int32)).to(dev), n_hops, Q=Q, kick=kick, slack=slack,
                            first_hop=first_hop, hist=hist)
    torch.cuda.current_stream(dev).synchronize()
    out = to_numpy(res)
    out["state"], out["best_state"] = out["state"].reshape(s.shape), out["best_state"].reshape(s.shape)
    return out


FIELDS_TABU3D = FIELDS_TABU + ("flags",)


def _block_tabu3d(N, Q, n, n_iters, tenure, tenure_rand, tenure_conf, first_iter):
    q = abi.Tabu3d()
    q.N, q.n_queens, q.n_chains, q.n_iters, q.first_iter = int(N), int(Q), int(n), int(n_iters), int(first_iter)
    q.tenure, q.tenure_rand, q.tenure_conf = int(tenure), int(tenure_rand), int(tenure_conf)
    return q


def tabu_queens_host(N, states, seeds, n_iters, Q=None, tenure=10, tenure_rand=0, tenure_conf=0, first_iter=0, tabu_in=None, best_floor=None,
                     hist=False, tabu_out=False):
    """mcq_tabu3d_host: tabu search of full_3d placements in the library's plain host code, NumPy in and out, no GPU.  Same result as
    tabu_queens, and it runs every shape (the kernel stops where a chain no longer fits the LDS: abi.tabu3d_lds_bytes)."""
    s = _host_queens(N, states, Q)
    n = s.shape[0]
    sd = _hop_seeds(seeds, n)
    q = _block_tabu3d(N, _queens_of(N, Q), n, n_iters, tenure, tenure_rand, tenure_conf, first_iter)
    width, cube = max(int(n_iters), 0) + 1, max(int(N), 0) ** 3
    out = _host_outputs(q, s, abi.TABU3D_DTYPES, {"energy_hist": (n, width), "tabu_out": (n, cube)}, _tabu_skip(hist, tabu_out), like=("best_state",))
    q.seeds, q.hist_stride = sd.ctypes.data, width
    keep = []
    if tabu_in is not None:
        keep.append(np.ascontiguousarray(tabu_in, dtype=np.uint16).reshape(-1))
        if keep[-1].shape[0] != n * cube:
            raise ValueError(f"tabu_in must be uint16[n_chains = {n}][N^3 = {cube}], got {np.shape(tabu_in)}")
        q.tabu_in = keep[-1].ctypes.data
    if best_floor is not None:
        keep.append(np.ascontiguousarray(best_floor, dtype=np.int32).reshape(-1))
        if keep[-1].shape[0] != n:
            raise ValueError(f"best_floor must be int32[n_chains = {n}], got {np.shape(best_floor)}")
        q.best_floor = keep[-1].ctypes.data
    _lib.tabu3d_host(q)
    return out


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
    import torch

    n, Qn = _device_queens("tabu_queens_device", N, states, Q)
    dev = states.device
    if not (isinstance(seeds, torch.Tensor) and seeds.device == dev and seeds.dtype in (torch.int32, getattr(torch, "uint32", torch.int32)) and seeds.is_contiguous()
            and tuple(seeds.shape) == (n,)):
        raise ValueError(f"tabu_queens_device takes seeds as a contiguous int32 or uint32 tensor [n_chains = {n}] on the device of states")
    cube = max(int(N), 0) ** 3
    if tabu_in is not None and not (isinstance(tabu_in, torch.Tensor) and tabu_in.device == dev and tabu_in.is_contiguous() and tabu_in.numel() == n * cube
                                    and tabu_in.dtype in (torch.int16, getattr(torch, "uint16", torch.int16))):
        raise ValueError(f"tabu_queens_device takes tabu_in as a contiguous int16 or uint16 tensor [n_chains = {n}][N^3 = {cube}] on the device of states")
    if best_floor is not None and not (isinstance(best_floor, torch.Tensor) and best_floor.device == dev and best_floor.is_contiguous()
                                       and best_floor.dtype == torch.int32 and tuple(best_floor.shape) == (n,)):
        raise ValueError(f"tabu_queens_device takes best_floor as a contiguous int32 tensor [n_chains = {n}] on the device of states")
    st = torch.cuda.current_stream(dev) if stream is None else stream
    with torch.cuda.device(dev), torch.cuda.stream(st):
        q = _block_tabu3d(N, Qn, n, n_iters, tenure, tenure_rand, tenure_conf, first_iter)
        width = max(int(n_iters), 0) + 1
        res = {"state": _device_out(out, states), "best_state": torch.empty_like(states)}
        for k, dt in abi.TABU3D_DTYPES.items():
            if k == "energy_hist":
                if hist:
                    res[k] = torch.empty((n, width), dtype=torch.int32, device=dev)
            elif k == "tabu_out":
                if tabu_out:
                    res[k] = torch.empty((n, cube), dtype=torch.int16, device=dev)
            else:
                res[k] = torch.empty(n, dtype=torch.int64 if dt is np.int64 else torch.int32, device=dev)
        q.seeds, q.state_in, q.state_out, q.best_state, q.hist_stride = seeds.data_ptr(), states.data_ptr(), res["state"].data_ptr(), res["best_state"].data_ptr(), width
        if tabu_in is not None:
            q.tabu_in = tabu_in.data_ptr()
        if best_floor is not None:
            q.best_floor = best_floor.data_ptr()
        for k in abi.TABU3D_DTYPES:
            if k in res:
                setattr(q, k, res[k].data_ptr())
        _lib.tabu3d_device(q, st)
    return res


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
    import torch

    s = _host_queens(N, states, Q)
    sd = _hop_seeds(seeds, s.shape[0])
    kw = dict(Q=Q, tenure=tenure, tenure_rand=tenure_rand, tenure_conf=tenure_conf, first_iter=first_iter, hist=hist, tabu_out=tabu_out)
    if s.shape[0] == 0:
        _lib.tabu3d_host(_block_tabu3d(N, _queens_of(N, Q), 0, n_iters, tenure, tenure_rand, tenure_conf, first_iter))  # raises the library's refusal
    if abi.MIN_N <= int(N) <= abi.MAX_N_QUENCH3D and abi.tabu3d_lds_bytes(N, Q) > abi.MAX_TABU3D_LDS:
        return tabu_queens_host(N, s, sd, n_iters, tabu_in=tabu_in, best_floor=best_floor, **kw)
    dev = torch.device("cuda", torch.cuda.current_device())
    ti = None if tabu_in is None else torch.from_numpy(np.ascontiguousarray(tabu_in, dtype=np.uint16).view(np.int16)).to(dev)
    bf = None if best_floor is None else torch.from_numpy(np.ascontiguousarray(best_floor, dtype=np.int32)).to(dev)
    res = tabu_queens_device(N, torch.from_numpy(s).to(dev), torch.from_numpy(sd.view(np.int32)).to(dev), n_iters, tabu_in=ti, best_floor=bf, **kw)
    torch.cuda.current_stream(dev).synchronize()
    out = tabu_to_numpy(res)
    out["state"], out["best_state"] = out["state"].reshape(s.shape), out["best_state"].reshape(s.shape)
    return out


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
