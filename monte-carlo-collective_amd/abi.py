"""ctypes mirror of include/mcq.h (the C-ABI under run_experiment).

Everything here is plain data: the structs, the enum values, and the mapping from the
reference's string vocabulary (`mcmc_type`, `init_mode`, `betta_scheduling.type`;
experiments.py:79-105, 497-502; mcmc_board.py:26-59) to those enums.
"""
import ctypes as C

import numpy as np

ABI_VERSION = 6

OK, EINVAL, EDEVICE, ENOMEM = 0, -1, -2, -3

MODE_BOARD, MODE_FULL3D = 0, 1
INIT = {"random": 0, "latin": 1, "klarner": 2}
SCHED = {
    "constant": 0,
    "linear_annealing": 1,
    "exponential_annealing": 2,
    "logarithmic_annealing": 3,
    "sinusoidal_annealing": 4,
}
RNG_MT19937_NUMPY = 0
RNG_PHILOX4X32_10 = 1
RNG = {"mt19937": RNG_MT19937_NUMPY, "numpy": RNG_MT19937_NUMPY, "philox": RNG_PHILOX4X32_10}
TRACE_NONE, TRACE_I32, TRACE_REDUCED = 0, 1, 2
FLAG_EXACT_EXP = 1
FLAG_SEQUENTIAL_DRAWS = 2
FLAG_LINE_COUNTERS = 4  # HIP: dE from per-line occupancy counters in LDS (boards up to N = 8 at 4 lanes per chain)
FLAG_SHARED_PACING = 16  # HIP: pace against every launch of the process that sets the flag (one progress table per device)
FLAG_PRIORITY_SHIFT = 8  # bits 8..9: s_setprio level of a small launch's wavefronts (include/mcq.h: MCQ_FLAG_PRIORITY)


def flag_priority(p):
    return (int(p) & 3) << FLAG_PRIORITY_SHIFT


# mcq_sweep_variant: the template arguments of mcq_sweep_kernel, in the kernel's order
SWEEP_VARIANT_FIELDS = ("MODE", "G", "PATIENCE", "NT", "REDUCED", "PHILOX", "NC", "EXCH", "CAND5", "EARLYU", "SLIM", "CNT", "WIDE")
MIN_N, MAX_N, MAX_N_BOARD = 2, 64, 128  # include/mcq.h: full_3d up to 64, boards up to 128
MAX_HIST_STRIDE = 1 << 24  # a full trace row (hist_stride entries) must stay below this: include/mcq.h


class Schedule(C.Structure):
    """include/mcq.h: mcq_schedule -- one beta schedule of a batched run"""
    _fields_ = [
        ("sched", C.c_int32),
        ("init_plus1", C.c_int32),
        ("beta_const", C.c_double),
        ("beta_start", C.c_double),
        ("beta_end", C.c_double),
    ]


class Params(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int32),
        ("N", C.c_int32),
        ("mode", C.c_int32),
        ("init", C.c_int32),
        ("sched", C.c_int32),
        ("rng", C.c_int32),
        ("trace", C.c_int32),
        ("flags", C.c_uint32),
        ("beta_const", C.c_double),
        ("beta_start", C.c_double),
        ("beta_end", C.c_double),
        ("n_steps", C.c_int64),
        ("n_chains", C.c_int64),
        ("patience", C.c_int64),
        ("hist_stride", C.c_int64),
        ("bits_stride", C.c_int64),
        ("lanes_per_chain", C.c_int32),
        ("device", C.c_int32),
        ("n_sets", C.c_int64),
        ("chains_per_set", C.c_int64),
        ("sets", C.POINTER(Schedule)),
        ("beta_table", C.c_void_p),
        ("exchange_every", C.c_int64),
        ("exchange_replicas", C.c_int32),
        ("n_queens", C.c_int32),
        ("exchange_ladder", C.POINTER(C.c_double)),
        ("stream_states", C.c_void_p),
    ]


class Resume(C.Structure):
    """include/mcq.h: mcq_resume -- the segment of a longer schedule a call runs, and what it starts from"""
    _fields_ = [
        ("first_step", C.c_int64),
        ("schedule_steps", C.c_int64),
        ("state", C.c_void_p),
        ("stream", C.c_void_p),
    ]


MAX_POPULATION = 1 << 19       # include/mcq.h: MCQ_MAX_POPULATION
MAX_RESAMPLE_TABLE = 1 << 16   # MCQ_MAX_RESAMPLE_TABLE
RESAMPLE_WEIGHT_BITS = 24      # MCQ_RESAMPLE_WEIGHT_BITS


class Resample(C.Structure):
    """include/mcq.h: mcq_resample -- one resampling boundary of population annealing"""
    _fields_ = [
        ("n_chains", C.c_int64),
        ("population", C.c_int64),
        ("state_bytes", C.c_int64),
        ("table", C.c_void_p),
        ("table_len", C.c_int64),
        ("offsets", C.c_void_p),
        ("energies", C.c_void_p),
        ("state_in", C.c_void_p),
        ("state_out", C.c_void_p),
        ("parent", C.c_void_p),
        ("stats", C.c_void_p),
        ("energy_out", C.c_void_p),
        ("first_step", C.c_int64),
        ("seg_best_energy", C.c_void_p),
        ("seg_steps_to_best", C.c_void_p),
        ("seg_n_accepted", C.c_void_p),
        ("seg_near_ties", C.c_void_p),
        ("seg_stream_words", C.c_void_p),
        ("seg_best_state", C.c_void_p),
        ("run_best_energy", C.c_void_p),
        ("run_steps_to_best", C.c_void_p),
        ("run_n_accepted", C.c_void_p),
        ("run_near_ties", C.c_void_p),
        ("run_stream_words", C.c_void_p),
        ("run_best_state", C.c_void_p),
    ]


def resample_table(dbeta):
    """The weight table of one boundary (include/mcq.h, population annealing, step 2): T[d] = floor(2^24 exp(-dbeta d)) as uint32 for
    d = 0 .. D - 1, D = 1 + the first d with T = 0, at most 2^16.  NumPy's exp / floor on float64."""
    dbeta = float(dbeta)
    if not dbeta >= 0.0:
        raise ValueError(f"population annealing needs a schedule that does not decrease: a boundary has dbeta = {dbeta}")
    d = np.arange(MAX_RESAMPLE_TABLE, dtype=np.float64)
    t = np.floor(float(1 << RESAMPLE_WEIGHT_BITS) * np.exp(-dbeta * d)).astype(np.uint32)
    zero = np.flatnonzero(t == 0)
    return np.ascontiguousarray(t[: int(zero[0]) + 1] if len(zero) else t)


class Quench(C.Structure):
    """include/mcq.h: mcq_quench -- the zero-temperature descent of board placements to a local minimum"""
    _fields_ = [
        ("N", C.c_int32),
        ("mode", C.c_int32),
        ("n_chains", C.c_int64),
        ("max_passes", C.c_int64),
        ("state_in", C.c_void_p),
        ("state_out", C.c_void_p),
        ("energy_in", C.c_void_p),
        ("energy_out", C.c_void_p),
        ("n_moves", C.c_void_p),
        ("n_passes", C.c_void_p),
        ("conflicts", C.c_void_p),
    ]


# the per-chain outputs of a quench besides the placements: field -> dtype ("conflicts" has a row of N*N per chain)
QUENCH_DTYPES = {"energy_in": np.int32, "energy_out": np.int32, "n_moves": np.int32, "n_passes": np.int32, "conflicts": np.uint16}


MAX_N_QUENCH_PAIRS = 32        # include/mcq.h: MCQ_MAX_N_QUENCH_PAIRS


class QuenchPairs(C.Structure):
    """include/mcq.h: mcq_quench_pairs -- the descent of board placements under single-height moves and moves of two aligned columns"""
    _fields_ = [
        ("N", C.c_int32),
        ("mode", C.c_int32),
        ("n_chains", C.c_int64),
        ("max_rounds", C.c_int64),
        ("state_in", C.c_void_p),
        ("state_out", C.c_void_p),
        ("energy_in", C.c_void_p),
        ("energy_single", C.c_void_p),
        ("energy_out", C.c_void_p),
        ("n_moves", C.c_void_p),
        ("n_pair_moves", C.c_void_p),
        ("n_rounds", C.c_void_p),
        ("certified", C.c_void_p),
        ("conflicts", C.c_void_p),
    ]


# the per-chain outputs of a pair-move quench besides the placements: field -> dtype ("conflicts" has a row of N*N per chain)
QUENCH_PAIRS_DTYPES = {"energy_in": np.int32, "energy_single": np.int32, "energy_out": np.int32, "n_moves": np.int32, "n_pair_moves": np.int32,
                       "n_rounds": np.int32, "certified": np.int32, "conflicts": np.uint16}


HOP_SINGLE, HOP_PAIRS = 0, 1   # include/mcq.h: MCQ_HOP_SINGLE, MCQ_HOP_PAIRS
MAX_HOP_KICK = 1024            # MCQ_MAX_HOP_KICK
HOP_LOCAL_SEARCH = {"single": HOP_SINGLE, "pairs": HOP_PAIRS}


class Hop(C.Structure):
    """include/mcq.h: mcq_hop -- basin hopping of board placements: kick, local search, keep the new minimum when it is no worse"""
    _fields_ = [
        ("N", C.c_int32),
        ("mode", C.c_int32),
        ("n_chains", C.c_int64),
        ("n_hops", C.c_int64),
        ("first_hop", C.c_int64),
        ("kick", C.c_int32),
        ("slack", C.c_int32),
        ("local_search", C.c_int32),
        ("seeds", C.c_void_p),
        ("state_in", C.c_void_p),
        ("state_out", C.c_void_p),
        ("energy_in", C.c_void_p),
        ("energy_start", C.c_void_p),
        ("energy_out", C.c_void_p),
        ("best_energy", C.c_void_p),
        ("best_hop", C.c_void_p),
        ("best_state", C.c_void_p),
        ("n_accepted", C.c_void_p),
        ("n_improved", C.c_void_p),
        ("n_moves", C.c_void_p),
        ("n_pair_moves", C.c_void_p),
        ("energy_hist", C.c_void_p),
        ("hist_stride", C.c_int64),
    ]


# the per-chain outputs of a hop call besides the placements (state, best_state): field -> dtype ("energy_hist" has a row of n_hops + 1 per chain)
HOP_DTYPES = {"energy_in": np.int32, "energy_start": np.int32, "energy_out": np.int32, "best_energy": np.int32, "best_hop": np.int64,
              "n_accepted": np.int64, "n_improved": np.int64, "n_moves": np.int64, "n_pair_moves": np.int64, "energy_hist": np.int32}


MAX_N_QUENCH3D = 32            # include/mcq.h: MCQ_MAX_N_QUENCH3D
QUENCH3D_REPEATED = 1          # MCQ_QUENCH3D_REPEATED: bit 0 of flags


class Quench3D(C.Structure):
    """include/mcq.h: mcq_quench3d -- the zero-temperature descent of full_3d placements to a local minimum"""
    _fields_ = [
        ("N", C.c_int32),
        ("n_queens", C.c_int32),
        ("n_chains", C.c_int64),
        ("max_passes", C.c_int64),
        ("state_in", C.c_void_p),
        ("state_out", C.c_void_p),
        ("energy_in", C.c_void_p),
        ("energy_out", C.c_void_p),
        ("n_moves", C.c_void_p),
        ("n_passes", C.c_void_p),
        ("conflicts", C.c_void_p),
        ("flags", C.c_void_p),
    ]


# the per-chain outputs of a full_3d quench besides the placements: field -> dtype ("conflicts" has a row of Q per chain)
QUENCH3D_DTYPES = {"energy_in": np.int32, "energy_out": np.int32, "n_moves": np.int32, "n_passes": np.int32, "conflicts": np.uint16,
                   "flags": np.int32}


MAX_HOP3D_LDS = 160 * 1024     # include/mcq.h: MCQ_MAX_HOP3D_LDS
HOP3D_REPEATED = 1             # MCQ_HOP3D_REPEATED: bit 0 of flags


class Hop3d(C.Structure):
    """include/mcq.h: mcq_hop3d -- basin hopping of full_3d placements: kick queens to free cells, descend, keep the new minimum when it is no worse"""
    _fields_ = [
        ("N", C.c_int32),
        ("n_queens", C.c_int32),
        ("n_chains", C.c_int64),
        ("n_hops", C.c_int64),
        ("first_hop", C.c_int64),
        ("kick", C.c_int32),
        ("slack", C.c_int32),
        ("seeds", C.c_void_p),
        ("state_in", C.c_void_p),
        ("state_out", C.c_void_p),
        ("energy_in", C.c_void_p),
        ("energy_start", C.c_void_p),
        ("energy_out", C.c_void_p),
        ("best_energy", C.c_void_p),
        ("best_hop", C.c_void_p),
        ("best_state", C.c_void_p),
        ("n_accepted", C.c_void_p),
        ("n_improved", C.c_void_p),
        ("n_moves", C.c_void_p),
        ("n_passes", C.c_void_p),
        ("n_kicked", C.c_void_p),
        ("energy_hist", C.c_void_p),
        ("hist_stride", C.c_int64),
        ("flags", C.c_void_p),
    ]


# the per-chain outputs of a full_3d hop call besides the placements (state, best_state): field -> dtype ("energy_hist" has a row of n_hops + 1 per chain)
HOP3D_DTYPES = {"energy_in": np.int32, "energy_start": np.int32, "energy_out": np.int32, "best_energy": np.int32, "best_hop": np.int64,
                "n_accepted": np.int64, "n_improved": np.int64, "n_moves": np.int64, "n_passes": np.int64, "n_kicked": np.int64,
                "energy_hist": np.int32, "flags": np.int32}


def hop3d_lds_bytes(N, Q=None):
    """The bytes of LDS a chain of mcq_hop3d_device takes (include/mcq.h, below the rule): it runs what stays within MAX_HOP3D_LDS."""
    N = int(N)
    Q = N * N if Q is None or int(Q) == 0 else int(Q)
    cells, cpd = N ** 3, 4 if N <= 19 else 2
    return 4 * (32 + -(-cells // cpd) + -(-cells // 32) + 2 * ((Q + 1) // 2))


MAX_TABU_TENURE = 8192         # include/mcq.h: MCQ_MAX_TABU_TENURE
MAX_TABU_TENURE_RAND = 4095    # MCQ_MAX_TABU_TENURE_RAND
MAX_TABU_TENURE_CONF = 64      # MCQ_MAX_TABU_TENURE_CONF
MAX_TABU_LDS = 160 * 1024      # MCQ_MAX_TABU_LDS


class Tabu(C.Structure):
    """include/mcq.h: mcq_tabu -- tabu search of board placements: the best admissible move of a conflicting column, the way back forbidden for a while"""
    _fields_ = [
        ("N", C.c_int32),
        ("mode", C.c_int32),
        ("n_chains", C.c_int64),
        ("n_iters", C.c_int64),
        ("first_iter", C.c_int64),
        ("tenure", C.c_int32),
        ("tenure_rand", C.c_int32),
        ("tenure_conf", C.c_int32),
        ("seeds", C.c_void_p),
        ("state_in", C.c_void_p),
        ("state_out", C.c_void_p),
        ("tabu_in", C.c_void_p),
        ("tabu_out", C.c_void_p),
        ("best_floor", C.c_void_p),
        ("energy_in", C.c_void_p),
        ("energy_out", C.c_void_p),
        ("best_energy", C.c_void_p),
        ("best_iter", C.c_void_p),
        ("best_state", C.c_void_p),
        ("n_moves", C.c_void_p),
        ("n_aspired", C.c_void_p),
        ("n_uphill", C.c_void_p),
        ("n_stalled", C.c_void_p),
        ("energy_hist", C.c_void_p),
        ("hist_stride", C.c_int64),
    ]


# the per-chain outputs of a tabu call besides the placements (state, best_state): field -> dtype ("energy_hist" has a row of n_iters + 1
# per chain, "tabu_out" one of N^3)
TABU_DTYPES = {"energy_in": np.int32, "energy_out": np.int32, "best_energy": np.int32, "best_iter": np.int64, "n_moves": np.int64,
               "n_aspired": np.int64, "n_uphill": np.int64, "n_stalled": np.int64, "energy_hist": np.int32, "tabu_out": np.uint16}


def tabu_lds_bytes(N):
    """The bytes of LDS a chain of mcq_tabu_device takes (include/mcq.h, below the rule): table, stamps, heights and best placement."""
    NP = next(p for p in (4, 8, 12, 16, 24, 32) if int(N) <= p)
    return NP * NP * (4 * ((NP // 4) | 1) + 4 * ((NP // 2) | 1) + 2)


MAX_TABU3D_SPAN = (1 << 14) - 1  # include/mcq.h: MCQ_MAX_TABU3D_SPAN
MAX_TABU3D_LDS = 160 * 1024    # MCQ_MAX_TABU3D_LDS
TABU3D_REPEATED = 1            # MCQ_TABU3D_REPEATED: bit 0 of flags


class Tabu3d(C.Structure):
    """include/mcq.h: mcq_tabu3d -- tabu search of full_3d placements: the best admissible move of a conflicting queen, the cell left forbidden for a while"""
    _fields_ = [
        ("N", C.c_int32),
        ("n_queens", C.c_int32),
        ("n_chains", C.c_int64),
        ("n_iters", C.c_int64),
        ("first_iter", C.c_int64),
        ("tenure", C.c_int32),
        ("tenure_rand", C.c_int32),
        ("tenure_conf", C.c_int32),
        ("seeds", C.c_void_p),
        ("state_in", C.c_void_p),
        ("state_out", C.c_void_p),
        ("tabu_in", C.c_void_p),
        ("tabu_out", C.c_void_p),
        ("best_floor", C.c_void_p),
        ("energy_in", C.c_void_p),
        ("energy_out", C.c_void_p),
        ("best_energy", C.c_void_p),
        ("best_iter", C.c_void_p),
        ("best_state", C.c_void_p),
        ("n_moves", C.c_void_p),
        ("n_aspired", C.c_void_p),
        ("n_uphill", C.c_void_p),
        ("n_stalled", C.c_void_p),
        ("energy_hist", C.c_void_p),
        ("hist_stride", C.c_int64),
        ("flags", C.c_void_p),
    ]


# the per-chain outputs of a full_3d tabu call besides the placements (state, best_state): field -> dtype ("energy_hist" has a row of
# n_iters + 1 per chain, "tabu_out" one of N^3)
TABU3D_DTYPES = dict(TABU_DTYPES, flags=np.int32)


def tabu3d_lds_bytes(N, Q=None):
    """The bytes of LDS a chain of mcq_tabu3d_device takes (include/mcq.h, below the rule): it runs what stays within MAX_TABU3D_LDS."""
    N = int(N)
    Q = N * N if Q is None or int(Q) == 0 else int(Q)
    cells, cpd = N ** 3, 4 if N <= 19 else 2
    return 4 * (32 + -(-cells // 2) + -(-cells // cpd) + -(-cells // 32) + (Q + 1) // 2)


MAX_RELINK_LDS = 160 * 1024    # include/mcq.h: MCQ_MAX_RELINK_LDS


class Relink(C.Structure):
    """include/mcq.h: mcq_relink -- path relinking between board placements: walk towards a guide, the best placement on the way to the local search"""
    _fields_ = [
        ("N", C.c_int32),
        ("mode", C.c_int32),
        ("n_chains", C.c_int64),
        ("max_steps", C.c_int32),
        ("min_dist", C.c_int32),
        ("local_search", C.c_int32),
        ("walk", C.c_int64),
        ("seeds", C.c_void_p),
        ("state_in", C.c_void_p),
        ("guide_in", C.c_void_p),
        ("state_out", C.c_void_p),
        ("path_best_state", C.c_void_p),
        ("distance_in", C.c_void_p),
        ("n_steps", C.c_void_p),
        ("path_best_step", C.c_void_p),
        ("energy_in", C.c_void_p),
        ("path_best_energy", C.c_void_p),
        ("path_max_energy", C.c_void_p),
        ("energy_out", C.c_void_p),
        ("n_moves", C.c_void_p),
        ("n_pair_moves", C.c_void_p),
        ("energy_hist", C.c_void_p),
        ("hist_stride", C.c_int64),
    ]


# the per-chain outputs of a relink call besides the placements (state, path_best_state): field -> dtype ("energy_hist" has a row of
# W + 1 per chain, W = max_steps or N^2)
RELINK_DTYPES = {"distance_in": np.int32, "n_steps": np.int32, "path_best_step": np.int32, "energy_in": np.int32, "path_best_energy": np.int32,
                 "path_max_energy": np.int32, "energy_out": np.int32, "n_moves": np.int64, "n_pair_moves": np.int64, "energy_hist": np.int32}


def relink_lds_bytes(N, pairs=True):
    """The bytes of LDS a chain of mcq_relink_device takes (include/mcq.h, below the rule): table, three placements and the scan's masks."""
    NP = next(p for p in (4, 8, 12, 16, 24, 32) if int(N) <= p)
    return NP * NP * (4 * ((NP // 4) | 1) + 3) + (8 * NP * NP if pairs else 0)


MAX_RELINK3D_LDS = 160 * 1024    # include/mcq.h: MCQ_MAX_RELINK3D_LDS
RELINK3D_REPEATED = 1            # MCQ_RELINK3D_REPEATED: bit 0 of flags, a repeated state_in
RELINK3D_GUIDE_REPEATED = 2      # MCQ_RELINK3D_GUIDE_REPEATED: bit 1 of flags, a repeated guide_in


class Relink3d(C.Structure):
    """include/mcq.h: mcq_relink3d -- path relinking between full_3d placements: walk towards a guide's cells, the best placement on the way to the descent"""
    _fields_ = [
        ("N", C.c_int32),
        ("n_queens", C.c_int32),
        ("n_chains", C.c_int64),
        ("max_steps", C.c_int32),
        ("min_dist", C.c_int32),
        ("walk", C.c_int64),
        ("seeds", C.c_void_p),
        ("state_in", C.c_void_p),
        ("guide_in", C.c_void_p),
        ("state_out", C.c_void_p),
        ("path_best_state", C.c_void_p),
        ("distance_in", C.c_void_p),
        ("n_steps", C.c_void_p),
        ("path_best_step", C.c_void_p),
        ("energy_in", C.c_void_p),
        ("path_best_energy", C.c_void_p),
        ("path_max_energy", C.c_void_p),
        ("energy_out", C.c_void_p),
        ("n_moves", C.c_void_p),
        ("n_passes", C.c_void_p),
        ("energy_hist", C.c_void_p),
        ("hist_stride", C.c_int64),
        ("flags", C.c_void_p),
    ]


# the per-chain outputs of a full_3d relink call besides the placements (state, path_best_state): field -> dtype ("energy_hist" has a
# row of W + 1 per chain, W = max_steps or Q)
RELINK3D_DTYPES = {"distance_in": np.int32, "n_steps": np.int32, "path_best_step": np.int32, "energy_in": np.int32, "path_best_energy": np.int32,
                   "path_max_energy": np.int32, "energy_out": np.int32, "n_moves": np.int64, "n_passes": np.int64, "energy_hist": np.int32,
                   "flags": np.int32}


def relink3d_lds_bytes(N, Q=None):
    """The bytes of LDS a chain of mcq_relink3d_device takes (include/mcq.h, below the rule): it runs what stays within MAX_RELINK3D_LDS."""
    N = int(N)
    Q = N * N if Q is None or int(Q) == 0 else int(Q)
    cells, cpd = N ** 3, 4 if N <= 19 else 2
    D = min(Q, cells - Q)  # the entries of the lists of moving queens and open targets
    return 4 * (32 + 2 * -(-cells // 32) + -(-cells // cpd) + 2 * ((Q + 1) // 2) + 2 * ((D + 1) // 2))


MAX_NFOLD_TABLE = 128          # include/mcq.h: MCQ_MAX_NFOLD_TABLE
NFOLD_TIME_BITS = 12           # MCQ_NFOLD_TIME_BITS: time is counted in units of 2^-12 Metropolis step
NFOLD_WEIGHT_BITS = 24         # MCQ_NFOLD_WEIGHT_BITS: no entry of a weight row exceeds 2^24
NFOLD_CLOCK_BITS = 26          # MCQ_NFOLD_CLOCK_BITS: no entry of the clock table exceeds 2^26
NFOLD_NEED_BITS = 45           # MCQ_NFOLD_NEED_BITS: need < 2^45
NFOLD_STEP_BITS = 50           # MCQ_NFOLD_STEP_BITS: (first_seg + n_segs) seg_steps < 2^50


class Nfold(C.Structure):
    """include/mcq.h: mcq_nfold -- the n-fold way for board placements: the Metropolis dynamics without its rejections"""
    _fields_ = [
        ("N", C.c_int32),
        ("mode", C.c_int32),
        ("n_chains", C.c_int64),
        ("n_segs", C.c_int64),
        ("first_seg", C.c_int64),
        ("seg_steps", C.c_int64),
        ("seeds", C.c_void_p),
        ("table", C.c_void_p),
        ("table_len", C.c_int64),
        ("clock_table", C.c_void_p),
        ("clock_ln2", C.c_int64),
        ("need_in", C.c_void_p),
        ("events_in", C.c_void_p),
        ("state_in", C.c_void_p),
        ("state_out", C.c_void_p),
        ("best_state", C.c_void_p),
        ("energy_in", C.c_void_p),
        ("energy_out", C.c_void_p),
        ("best_energy", C.c_void_p),
        ("best_step", C.c_void_p),
        ("events_out", C.c_void_p),
        ("n_uphill", C.c_void_p),
        ("n_flat", C.c_void_p),
        ("need_out", C.c_void_p),
        ("weight_out", C.c_void_p),
        ("energy_hist", C.c_void_p),
        ("hist_stride", C.c_int64),
    ]


# the per-chain outputs of an n-fold call besides the placements (state, best_state): field -> dtype ("energy_hist" has a row of
# n_segs + 1 per chain)
NFOLD_DTYPES = {"energy_in": np.int32, "energy_out": np.int32, "best_energy": np.int32, "best_step": np.int64, "events_out": np.int64,
                "n_uphill": np.int64, "n_flat": np.int64, "need_out": np.uint64, "weight_out": np.uint64, "energy_hist": np.int32}


MAX_NFOLD3D_TABLE = 512        # include/mcq.h: MCQ_MAX_NFOLD3D_TABLE
NFOLD3D_NEED_BITS = 58         # MCQ_NFOLD3D_NEED_BITS: need < 2^58
MAX_NFOLD3D_LDS = 160 * 1024   # MCQ_MAX_NFOLD3D_LDS
NFOLD3D_REPEATED = 1           # MCQ_NFOLD3D_REPEATED: bit 0 of flags


class Nfold3d(C.Structure):
    """include/mcq.h: mcq_nfold3d -- the n-fold way for full_3d placements: the Metropolis dynamics of a queen's move to a free cell without its rejections"""
    _fields_ = [
        ("N", C.c_int32),
        ("mode", C.c_int32),
        ("n_queens", C.c_int32),
        ("n_chains", C.c_int64),
        ("n_segs", C.c_int64),
        ("first_seg", C.c_int64),
        ("seg_steps", C.c_int64),
        ("seeds", C.c_void_p),
        ("table", C.c_void_p),
        ("table_len", C.c_int64),
        ("clock_table", C.c_void_p),
        ("clock_ln2", C.c_int64),
        ("need_in", C.c_void_p),
        ("events_in", C.c_void_p),
        ("state_in", C.c_void_p),
        ("state_out", C.c_void_p),
        ("best_state", C.c_void_p),
        ("energy_in", C.c_void_p),
        ("energy_out", C.c_void_p),
        ("best_energy", C.c_void_p),
        ("best_step", C.c_void_p),
        ("events_out", C.c_void_p),
        ("n_uphill", C.c_void_p),
        ("n_flat", C.c_void_p),
        ("need_out", C.c_void_p),
        ("weight_out", C.c_void_p),
        ("energy_hist", C.c_void_p),
        ("hist_stride", C.c_int64),
        ("flags", C.c_void_p),
    ]


# the per-chain outputs of a full_3d n-fold call besides the placements (state, best_state): field -> dtype ("energy_hist" has a row of
# n_segs + 1 per chain)
NFOLD3D_DTYPES = dict(NFOLD_DTYPES, flags=np.int32)


def nfold3d_lds_bytes(N, Q=None):
    """The bytes of LDS a chain of mcq_nfold3d_device takes (include/mcq.h, below the rule): it runs what stays within MAX_NFOLD3D_LDS."""
    N = int(N)
    Q = N * N if Q is None or int(Q) == 0 else int(Q)
    cells, cpd = N ** 3, 4 if N <= 19 else 2
    return 4 * (2376 + 2 * Q + -(-cells // cpd) + -(-cells // 32) + (Q + 1) // 2)


EO_MOVE_BEST = 0               # include/mcq.h: MCQ_EO_MOVE_BEST
EO_MOVE_RANDOM = 1             # MCQ_EO_MOVE_RANDOM
MAX_EO_LDS = 64 * 1024         # MCQ_MAX_EO_LDS


class Eo(C.Structure):
    """include/mcq.h: mcq_eo -- extremal optimisation of board placements: the column at a drawn rank of local badness moves, whatever it costs"""
    _fields_ = [
        ("N", C.c_int32),
        ("mode", C.c_int32),
        ("n_chains", C.c_int64),
        ("n_iters", C.c_int64),
        ("first_iter", C.c_int64),
        ("move", C.c_int32),
        ("n_ranks", C.c_int32),
        ("seeds", C.c_void_p),
        ("rank_cdf", C.c_void_p),
        ("state_in", C.c_void_p),
        ("state_out", C.c_void_p),
        ("best_floor", C.c_void_p),
        ("energy_in", C.c_void_p),
        ("energy_out", C.c_void_p),
        ("best_energy", C.c_void_p),
        ("best_iter", C.c_void_p),
        ("best_state", C.c_void_p),
        ("n_moves", C.c_void_p),
        ("n_uphill", C.c_void_p),
        ("n_flat", C.c_void_p),
        ("n_free", C.c_void_p),
        ("n_idle", C.c_void_p),
        ("energy_hist", C.c_void_p),
        ("hist_stride", C.c_int64),
    ]


# the per-chain outputs of an extremal-optimisation call besides the placements (state, best_state): field -> dtype ("energy_hist" has
# a row of n_iters + 1 per chain)
EO_DTYPES = {"energy_in": np.int32, "energy_out": np.int32, "best_energy": np.int32, "best_iter": np.int64, "n_moves": np.int64,
             "n_uphill": np.int64, "n_flat": np.int64, "n_free": np.int64, "n_idle": np.int64, "energy_hist": np.int32}


def eo_lds_bytes(N):
    """The bytes of LDS a chain of mcq_eo_device takes (include/mcq.h, below the rule): table, heights, best placement and rank_cdf."""
    NP = next(p for p in (4, 8, 12, 16, 24, 32) if int(N) <= p)
    return NP * NP * (4 * ((NP // 4) | 1) + 6)


EO3D_MOVE_BEST = 0             # include/mcq.h: MCQ_EO3D_MOVE_BEST
EO3D_MOVE_RANDOM = 1           # MCQ_EO3D_MOVE_RANDOM
MAX_EO3D_LDS = 160 * 1024      # MCQ_MAX_EO3D_LDS
EO3D_REPEATED = 1              # MCQ_EO3D_REPEATED: bit 0 of flags


class Eo3d(C.Structure):
    """include/mcq.h: mcq_eo3d -- extremal optimisation of full_3d placements: the queen at a drawn rank of local badness moves to a free cell, whatever it costs"""
    _fields_ = [
        ("N", C.c_int32),
        ("n_queens", C.c_int32),
        ("n_chains", C.c_int64),
        ("n_iters", C.c_int64),
        ("first_iter", C.c_int64),
        ("move", C.c_int32),
        ("n_ranks", C.c_int32),
        ("seeds", C.c_void_p),
        ("rank_cdf", C.c_void_p),
        ("state_in", C.c_void_p),
        ("state_out", C.c_void_p),
        ("best_floor", C.c_void_p),
        ("energy_in", C.c_void_p),
        ("energy_out", C.c_void_p),
        ("best_energy", C.c_void_p),
        ("best_iter", C.c_void_p),
        ("best_state", C.c_void_p),
        ("n_moves", C.c_void_p),
        ("n_uphill", C.c_void_p),
        ("n_flat", C.c_void_p),
        ("n_free", C.c_void_p),
        ("n_idle", C.c_void_p),
        ("energy_hist", C.c_void_p),
        ("hist_stride", C.c_int64),
        ("flags", C.c_void_p),
    ]


# the per-chain outputs of a full_3d extremal-optimisation call besides the placements (state, best_state): field -> dtype
# ("energy_hist" has a row of n_iters + 1 per chain)
EO3D_DTYPES = dict(EO_DTYPES, flags=np.int32)


def eo3d_lds_bytes(N, Q=None):
    """The bytes of LDS a chain of mcq_eo3d_device takes (include/mcq.h, below the rule); every shape stays within MAX_EO3D_LDS."""
    N = int(N)
    Q = N * N if Q is None or int(Q) == 0 else int(Q)
    cells, cpd = N ** 3, 4 if N <= 19 else 2
    return 4 * (480 + -(-cells // cpd) + -(-cells // 32) + (Q + 1) // 2)


MAX_HEATBATH_TABLE = 512       # include/mcq.h: MCQ_MAX_HEATBATH_TABLE
HEATBATH_WEIGHT_BITS = 24      # MCQ_HEATBATH_WEIGHT_BITS
MAX_N_HEATBATH_COUNTERS = 16   # MCQ_MAX_N_HEATBATH_COUNTERS: the largest N of mcq_heatbath_counters_device


class Heatbath(C.Structure):
    """include/mcq.h: mcq_heatbath -- heat-bath column sweeps of board placements"""
    _fields_ = [
        ("N", C.c_int32),
        ("mode", C.c_int32),
        ("n_chains", C.c_int64),
        ("n_sweeps", C.c_int64),
        ("first_sweep", C.c_int64),
        ("seeds", C.c_void_p),
        ("table", C.c_void_p),
        ("table_len", C.c_int64),
        ("state_in", C.c_void_p),
        ("state_out", C.c_void_p),
        ("energy_in", C.c_void_p),
        ("energy_out", C.c_void_p),
        ("best_energy", C.c_void_p),
        ("best_sweep", C.c_void_p),
        ("best_state", C.c_void_p),
        ("n_changed", C.c_void_p),
        ("energy_hist", C.c_void_p),
        ("hist_stride", C.c_int64),
    ]


# the per-chain outputs of a heat-bath call besides the placements: field -> dtype
HEATBATH_DTYPES = {"energy_in": np.int32, "energy_out": np.int32, "best_energy": np.int32, "best_sweep": np.int64, "n_changed": np.int64}


def heatbath_table(betas):
    """The weight rows of a heat-bath call (include/mcq.h, heat-bath rule, step 3): T[s][d] = floor(2^24 exp(-beta_s d)) as uint32 for
    d = 0 .. D - 1, one row per sweep; D = 1 + the first d with T = 0 over the rows, at most 512, the rows zero-padded.  NumPy's exp /
    floor on float64.  No sweep gives one row [2^24] that no sweep reads.  No entry exceeds 2^HEATBATH_WEIGHT_BITS, the bound the rule
    sets for every table, a caller's own included (the host entry points refuse a larger entry; the device ones cannot look)."""
    b = np.ascontiguousarray(betas, dtype=np.float64).reshape(-1)
    if not (np.isfinite(b).all() and (b >= 0.0).all()):
        raise ValueError("the heat-bath sweep needs finite beta >= 0 for every sweep")
    if b.size == 0:
        return np.full((1, 1), 1 << HEATBATH_WEIGHT_BITS, dtype=np.uint32)
    d = np.arange(MAX_HEATBATH_TABLE, dtype=np.float64)
    t = np.floor(float(1 << HEATBATH_WEIGHT_BITS) * np.exp(-b[:, None] * d[None, :])).astype(np.uint32)
    support = int((t != 0).any(axis=0).sum())  # the rows fall monotonically: the first all-zero d
    return np.ascontiguousarray(t[:, : min(support + 1, MAX_HEATBATH_TABLE)])


HEATBATH3D_REPEATED = 1        # include/mcq.h: MCQ_HEATBATH3D_REPEATED: bit 0 of flags


class Heatbath3D(C.Structure):
    """include/mcq.h: mcq_heatbath3d -- heat-bath queen sweeps of full_3d placements"""
    _fields_ = [
        ("N", C.c_int32),
        ("n_queens", C.c_int32),
        ("n_chains", C.c_int64),
        ("n_sweeps", C.c_int64),
        ("first_sweep", C.c_int64),
        ("seeds", C.c_void_p),
        ("table", C.c_void_p),
        ("table_len", C.c_int64),
        ("state_in", C.c_void_p),
        ("state_out", C.c_void_p),
        ("energy_in", C.c_void_p),
        ("energy_out", C.c_void_p),
        ("best_energy", C.c_void_p),
        ("best_sweep", C.c_void_p),
        ("best_state", C.c_void_p),
        ("n_changed", C.c_void_p),
        ("energy_hist", C.c_void_p),
        ("hist_stride", C.c_int64),
        ("flags", C.c_void_p),
    ]


# the per-chain outputs of a full_3d heat-bath call besides the placements: field -> dtype
HEATBATH3D_DTYPES = dict(HEATBATH_DTYPES, flags=np.int32)


MAX_TEMPER_SWAP_TABLE = 4096   # include/mcq.h: MCQ_MAX_TEMPER_SWAP_TABLE
MAX_TEMPER_LDS = 160 * 1024    # MCQ_MAX_TEMPER_LDS
TEMPER_REPLICAS = (2, 4, 8, 16)
MAX_N_TEMPER_COUNTERS = 16     # MCQ_MAX_N_TEMPER_COUNTERS: the largest N of mcq_temper_counters_device


class Temper(C.Structure):
    """include/mcq.h: mcq_temper -- parallel tempering of board heat-bath sweeps, one ladder per workgroup"""
    _fields_ = [
        ("N", C.c_int32),
        ("mode", C.c_int32),
        ("n_chains", C.c_int64),
        ("n_sweeps", C.c_int64),
        ("first_sweep", C.c_int64),
        ("replicas", C.c_int64),
        ("exchange_every", C.c_int64),
        ("n_events", C.c_int64),
        ("seeds", C.c_void_p),
        ("table", C.c_void_p),
        ("table_len", C.c_int64),
        ("swap_table", C.c_void_p),
        ("swap_len", C.c_int64),
        ("rung_in", C.c_void_p),
        ("rung_out", C.c_void_p),
        ("state_in", C.c_void_p),
        ("state_out", C.c_void_p),
        ("energy_in", C.c_void_p),
        ("energy_out", C.c_void_p),
        ("best_energy", C.c_void_p),
        ("best_sweep", C.c_void_p),
        ("best_state", C.c_void_p),
        ("n_changed", C.c_void_p),
        ("energy_hist", C.c_void_p),
        ("hist_stride", C.c_int64),
        ("n_exchanges", C.c_void_p),
        ("rung_hist", C.c_void_p),
        ("pair_accepted", C.c_void_p),
    ]


# the per-chain outputs of a tempered call besides the placements: field -> dtype (pair_accepted has a row of R - 1 per ladder)
TEMPER_DTYPES = dict(HEATBATH_DTYPES, rung_out=np.uint8, n_exchanges=np.int64)


TEMPER3D_HELD = 2              # include/mcq.h: MCQ_TEMPER3D_HELD: bit 1 of flags
TEMPER3D_STATIC_LDS = 256      # MCQ_TEMPER3D_STATIC_LDS


class Temper3D(C.Structure):
    """include/mcq.h: mcq_temper3d -- parallel tempering of full_3d heat-bath queen sweeps, one ladder per workgroup"""
    _fields_ = [("n_queens", t) if f == "mode" else (f, t) for f, t in Temper._fields_] + [("flags", C.c_void_p)]


# the per-chain outputs of a tempered full_3d call besides the placements
TEMPER3D_DTYPES = dict(TEMPER_DTYPES, flags=np.int32)


def temper3d_lds_bytes(N, R, Q=None, table_len=MAX_HEATBATH_TABLE):
    """The bytes of LDS a ladder of mcq_temper3d_device takes (include/mcq.h, below the rule): it runs what stays within
    MAX_TEMPER_LDS - TEMPER3D_STATIC_LDS."""
    N, R = int(N), int(R)
    Q = N * N if Q is None or int(Q) == 0 else int(Q)
    cells, cpd = N ** 3, 4 if N <= 19 else 2
    chain = (72 + -(-cells // cpd) + -(-cells // 32) + (Q + 1) // 2 + 3) // 4 * 4
    return 4 * (R * chain + R * int(table_len) + 3 * R)


def temper_counters_lds_bytes(N, R, table_len=MAX_HEATBATH_TABLE):
    """The bytes of LDS a workgroup of mcq_temper_counters_device takes (N <= MAX_N_TEMPER_COUNTERS), the arithmetic of its launch: per
    ladder R chain regions of the counter form -- (6 NP - 2)(5 NP - 2) counters and NP^2 heights, NP = N rounded up to 8, 12 or 16,
    rounded to 64 bytes off a multiple of 128: 1 856, 4 288 or 7 616 --, 4 R table_len bytes of staged rows and 12 R bytes for the
    event; two ladders where R = 2 (one is half a wavefront).  Never above MAX_TEMPER_LDS."""
    N, R = int(N), int(R)
    if not MIN_N <= N <= MAX_N_TEMPER_COUNTERS or R not in TEMPER_REPLICAS:
        raise ValueError(f"the counter form of the tempered sweep runs N = {MIN_N} .. {MAX_N_TEMPER_COUNTERS} with 2, 4, 8 or 16 replicas, got N = {N}, R = {R}")
    NP = 8 if N <= 8 else 12 if N <= 12 else 16
    chain = ((6 * NP - 2) * (5 * NP - 2) + NP * NP + 63) // 128 * 128 + 64
    return (2 if R == 2 else 1) * (R * chain + 4 * R * int(table_len) + 12 * R)


def temper_events(first_sweep, n_sweeps, exchange_every):
    """The exchange events of a call (include/mcq.h, tempering rule, item 3): floor((first_sweep + n_sweeps) / K) - floor(first_sweep / K)."""
    K = int(exchange_every)
    if K < 1:
        raise ValueError(f"exchange_every must be >= 1, got {exchange_every}")
    return (int(first_sweep) + int(n_sweeps)) // K - int(first_sweep) // K


def temper_ladder(ladder):
    """The multipliers l_0 <= .. <= l_{R-1} of a ladder as float64, checked: R in TEMPER_REPLICAS, finite, positive, non-decreasing (the
    one-sided swap table needs beta non-decreasing in the rung: rung R - 1 is the coldest)."""
    l = np.ascontiguousarray(ladder, dtype=np.float64).reshape(-1)
    if len(l) not in TEMPER_REPLICAS:
        raise ValueError(f"a ladder has 2, 4, 8 or 16 multipliers, got {len(l)}")
    if not (np.isfinite(l).all() and (l > 0.0).all()):
        raise ValueError("the multipliers of a ladder must be finite and positive")
    if (np.diff(l) < 0.0).any():
        raise ValueError("the multipliers of a ladder must be non-decreasing: a decreasing step would put the colder replica on the lower rung")
    return l


def temper_tables(betas, ladder, exchange_every=1, first_sweep=0):
    """Both tables of a tempered call (include/mcq.h, tempering rule, item 4), NumPy's exp / floor on float64:
      T uint32[n_sweeps][R][D]       T[s][t][d] = floor(2^24 exp(-beta_s l_t d)), the rows of heatbath_table at beta_s l_t; D as there;
      X uint32[n_events][R - 1][DX]  X[j][t][d] = min(2^32 - 1, floor(2^32 exp(-beta_g (l_{t+1} - l_t) d))), g the sweep event j follows;
                                     DX = 1 + the first d with X = 0 over the rows, at most MAX_TEMPER_SWAP_TABLE.
    A row of X whose exponent is 0 (beta_g = 0, or two equal multipliers) is constant and reads the same at every length; a positive
    exponent too small for the zero to arrive within MAX_TEMPER_SWAP_TABLE entries is a ValueError that names it: the kernel clamps d
    to DX - 1, and that entry must be the one every larger d has.  No sweep gives T = [[[2^24]] * R]; no event gives X of no rows."""
    l = temper_ladder(ladder)
    R = len(l)
    b = np.ascontiguousarray(betas, dtype=np.float64).reshape(-1)
    n_events = temper_events(first_sweep, b.size, exchange_every)  # (refuses K < 1)
    if int(first_sweep) < 0:
        raise ValueError(f"first_sweep must be >= 0, got {first_sweep}")
    if not (np.isfinite(b).all() and (b >= 0.0).all()):
        raise ValueError("the heat-bath sweep needs finite beta >= 0 for every sweep")
    if not np.isfinite(b[:, None] * l[None, :]).all():
        raise ValueError("beta times a ladder multiplier overflows")
    T = heatbath_table(b[:, None] * l[None, :]).reshape(max(b.size, 1), R if b.size else 1, -1)
    if b.size == 0:
        T = np.ascontiguousarray(np.repeat(T, R, axis=1))
    K = int(exchange_every)
    g = (int(first_sweep) // K + 1 + np.arange(n_events, dtype=np.int64)) * K - 1 - int(first_sweep)  # the call's sweep each event follows
    x = b[g][:, None] * np.diff(l)[None, :]  # [n_events][R - 1] exponents per unit of energy
    d = np.arange(MAX_TEMPER_SWAP_TABLE, dtype=np.float64)
    X = np.minimum(np.floor(4294967296.0 * np.exp(-x[:, :, None] * d[None, None, :])), 4294967295.0).astype(np.uint32)
    bad = (x > 0.0) & (X[:, :, -1] != 0)
    if bad.any():
        j, t = (int(v) for v in np.argwhere(bad)[0])
        raise ValueError(f"the ladder step l[{t + 1}] - l[{t}] = {l[t + 1] - l[t]:g} at beta = {b[g[j]]:g} (sweep {int(first_sweep) + int(g[j])}) is too small: "
                         f"exp(-{x[j, t]:g} d) does not reach 0 in 32 bits within swap_len = {MAX_TEMPER_SWAP_TABLE} entries")
    live = X[x > 0.0].reshape(-1, MAX_TEMPER_SWAP_TABLE)
    support = int((live != 0).any(axis=0).sum()) if live.size else 0  # the rows fall monotonically: the first all-zero d
    return T, np.ascontiguousarray(X[:, :, : min(support + 1, MAX_TEMPER_SWAP_TABLE)])


class PackSlot(C.Structure):
    """include/mcq.h: mcq_pack_slot -- where one job's fields sit in the packed summary tensor (word offsets, -1 = absent)"""
    _fields_ = [("counters", C.c_int64), ("min_slot", C.c_int64), ("best", C.c_int64), ("stb", C.c_int64), ("stats", C.c_int64)]


class Outputs(C.Structure):
    _fields_ = [
        ("energy_hist", C.c_void_p),
        ("accept_bits", C.c_void_p),
        ("hist_len", C.c_void_p),
        ("steps_executed", C.c_void_p),
        ("initial_energy", C.c_void_p),
        ("best_energy", C.c_void_p),
        ("final_energy", C.c_void_p),
        ("steps_to_best", C.c_void_p),
        ("n_accepted", C.c_void_p),
        ("near_ties", C.c_void_p),
        ("best_state", C.c_void_p),
        ("final_state", C.c_void_p),
        ("step_sum", C.c_void_p),
        ("step_sumsq", C.c_void_p),
        ("step_accepted", C.c_void_p),
        ("step_count", C.c_void_p),
        ("exchange_rung", C.c_void_p),
        ("n_exchanges", C.c_void_p),
        ("stream_words", C.c_void_p),
    ]


# field -> (dtype, per-chain shape builder)
OUTPUT_DTYPES = {
    "energy_hist": np.int32,
    "accept_bits": np.uint64,
    "hist_len": np.int64,
    "steps_executed": np.int64,
    "initial_energy": np.int32,
    "best_energy": np.int32,
    "final_energy": np.int32,
    "steps_to_best": np.int64,
    "n_accepted": np.int64,
    "near_ties": np.int64,
    "best_state": np.uint8,
    "final_state": np.uint8,
    "step_sum": np.int64,
    "step_sumsq": np.int64,
    "step_accepted": np.int64,
    "step_count": np.int64,
    "exchange_rung": np.int32,
    "n_exchanges": np.int64,
    "stream_words": np.uint32,
}


def state_bytes(N, mode, n_queens=0):
    """Bytes of one chain's state record: N*N heights (board) or Q*3 coordinates (full_3d; Q = N*N unless n_queens names a count)."""
    return N * N if mode == MODE_BOARD else 3 * (n_queens if n_queens else N * N)


def hist_stride_for(n_steps):
    """Row stride of energy_hist: n_steps + 1 entries rounded up to 64 (256-byte rows, so every
    64-entry block a wavefront flushes is one aligned 256-byte store)."""
    return ((n_steps + 1 + 63) // 64) * 64


def bits_stride_for(n_steps):
    return max(1, (n_steps + 63) // 64)


def output_shapes(p, trace=True, states=True):
    """name -> shape for the arrays a call with parameters `p` fills."""
    n = p.n_chains
    shapes = {k: (n,) for k in ("hist_len", "steps_executed", "initial_energy", "best_energy", "final_energy",
                                "steps_to_best", "n_accepted", "near_ties", "stream_words")}
    if isinstance(trace, str) and trace == "reduced":
        for k in ("step_sum", "step_sumsq", "step_accepted", "step_count"):
            shapes[k] = (p.n_sets, p.n_steps + 1) if p.n_sets > 1 else (p.n_steps + 1,)
    elif trace:
        shapes["energy_hist"] = (n, p.hist_stride)
        shapes["accept_bits"] = (n, p.bits_stride)
    if states:
        sb = state_bytes(p.N, p.mode, p.n_queens)
        shapes["best_state"] = (n, sb)
        shapes["final_state"] = (n, sb)
    if p.exchange_every > 0:
        shapes["exchange_rung"] = (n,)
        shapes["n_exchanges"] = (n,)
    return shapes


def trace_mode(trace):
    """True / False / "reduced" -> MCQ_TRACE_*"""
    if trace == "reduced":
        return TRACE_REDUCED
    return TRACE_I32 if trace else TRACE_NONE


def mode_of(mcmc_type):
    """experiments.py:497-502: "board" selects the board chain, anything else the full_3d chain."""
    return MODE_BOARD if mcmc_type == "board" else MODE_FULL3D


def normalise_patience(early_stop_patience):
    """experiments.py:284-285: None, 'None' and 'null' all disable early stopping."""
    if early_stop_patience in (None, "None", "null"):
        return -1
    v = int(early_stop_patience)
    return v if v >= 0 else 0  # a negative patience stops at the first step, like 0


def _check_schedule(schedule_params):
    """(type, beta_const, beta_start, beta_end) of a betta_scheduling dict; raises like the reference (experiments.py:85-105)"""
    if schedule_params is None:
        raise ValueError("schedule_params is required")
    st = schedule_params.get("type")
    if st not in SCHED:
        raise ValueError(f"Unknown betta_scheduling type: {st}")
    bc = schedule_params.get("beta_const")
    bs = schedule_params.get("beta_start")
    be = schedule_params.get("beta_end")
    if st == "constant":
        if bc is None:
            raise ValueError("beta_const required for constant schedule")
    elif bs is None or be is None:
        raise ValueError(f"beta_start and beta_end required for {st} schedule")
    f = lambda v: float(v) if v is not None else 0.0
    return st, f(bc), f(bs), f(be)


def make_params_sets(N, n_steps, init_mode, schedule_sets, chains_per_set, mcmc_type="full_3d", early_stop_patience=None,
                     trace=True, flags=0, lanes_per_chain=0, device=-1, rng="mt19937", init_modes=None):
    """Parameters of ONE launch that runs `chains_per_set` chains under each schedule of `schedule_sets` (a list of
    betta_scheduling dicts): chains [t * chains_per_set, (t + 1) * chains_per_set) follow schedule t.  What
    run_beta_start_end_pairs does pair by pair (experiments.py:741-846), batched.  `init_modes` (optional, one per set) gives
    every set its own initial state: the (init_mode, N) cells of measure_min_energy_vs_N that share N."""
    sets = [_check_schedule(sp) for sp in schedule_sets]
    if not sets:
        raise ValueError("at least one schedule")
    if chains_per_set <= 0 or chains_per_set % 16:
        raise ValueError("chains_per_set must be a positive multiple of 16")
    p = make_params(N, n_steps, init_mode, schedule_sets[0], chains_per_set * len(sets), mcmc_type=mcmc_type,
                    early_stop_patience=early_stop_patience, trace=trace, flags=flags, lanes_per_chain=lanes_per_chain, device=device,
                    rng=rng)
    arr = (Schedule * len(sets))()
    if init_modes is not None:
        if len(init_modes) != len(sets):
            raise ValueError("init_modes needs one entry per schedule set")
        for im in init_modes:
            if im not in INIT:
                raise ValueError(f"Unknown init_mode: {im}")
    for t, (a, (st, bc, bs, be)) in enumerate(zip(arr, sets)):
        a.sched, a.init_plus1, a.beta_const, a.beta_start, a.beta_end = SCHED[st], 0 if init_modes is None else INIT[init_modes[t]] + 1, bc, bs, be
    p.n_sets, p.chains_per_set = len(sets), chains_per_set
    p.sets = C.cast(arr, C.POINTER(Schedule))
    p._sets_keepalive = arr  # the struct only holds a pointer
    p._schedules = [dict(sp) for sp in schedule_sets]
    return p


def make_params(N, n_steps, init_mode, schedule_params, n_chains, mcmc_type="full_3d", early_stop_patience=None,
                trace=True, flags=0, lanes_per_chain=0, device=-1, rng="mt19937", Q=None):
    """Build a Params from the reference's vocabulary.  Raises ValueError exactly where the
    reference does: unknown schedule type (experiments.py:105), missing beta parameters
    (experiments.py:85-102), unknown init_mode (mcmc_board.py:59, mcmc.py:104)."""
    if schedule_params is None:
        raise ValueError("schedule_params is required")
    st = schedule_params.get("type")
    if st not in SCHED:
        raise ValueError(f"Unknown betta_scheduling type: {st}")
    bc = schedule_params.get("beta_const")
    bs = schedule_params.get("beta_start")
    be = schedule_params.get("beta_end")
    if st == "constant":
        if bc is None:
            raise ValueError("beta_const required for constant schedule")
    elif bs is None or be is None:
        raise ValueError(f"beta_start and beta_end required for {st} schedule")
    if init_mode not in INIT:
        raise ValueError(f"Unknown init_mode: {init_mode}")
    N = int(N)
    top = MAX_N_BOARD if mode_of(mcmc_type) == MODE_BOARD else MAX_N
    if not (MIN_N <= N <= top):
        raise ValueError(f"N must be in [{MIN_N}, {top}] for mcmc_type {mcmc_type}, got {N}")
    n_steps = int(n_steps)
    if n_steps < 0:
        raise ValueError("n_steps must be >= 0")
    p = Params()
    p.abi_version = ABI_VERSION
    p.N = N
    p.mode = mode_of(mcmc_type)
    p.init = INIT[init_mode]
    p.sched = SCHED[st]
    if rng not in RNG:
        raise ValueError(f"Unknown rng: {rng}")
    p.rng = RNG[rng]
    p.trace = trace_mode(trace)
    p.flags = flags
    p.beta_const = float(bc) if bc is not None else 0.0
    p.beta_start = float(bs) if bs is not None else 0.0
    p.beta_end = float(be) if be is not None else 0.0
    p.n_steps = n_steps
    p.n_chains = int(n_chains)
    p.patience = normalise_patience(early_stop_patience) if p.mode == MODE_BOARD else -1
    p.hist_stride = hist_stride_for(n_steps)
    p.bits_stride = bits_stride_for(n_steps)
    p.lanes_per_chain = lanes_per_chain
    p.device = device
    p._schedules = [dict(schedule_params)]  # what abi.beta_table evaluates (the struct itself only holds enums and doubles)
    if Q is not None and int(Q) != N * N:  # State3DQueens(N, Q=...): mcmc.py:6-18
        Q = int(Q)
        if p.mode != MODE_FULL3D:
            raise ValueError("Q applies to mcmc_type full_3d (a board has one queen per column)")
        if init_mode in ("latin", "klarner"):
            raise ValueError(f"{init_mode} initialization assumes Q = N^2, got Q={Q}, N^2={N * N}.")  # mcmc.py:21-25
        if Q > N ** 3:
            raise ValueError(f"Q={Q} cannot exceed N^3={N ** 3}.")  # mcmc.py:94-95
        if Q < 2 or Q == N ** 3 or Q > 32767:
            raise ValueError(f"this build runs 2 <= Q < N^3 and Q <= 32767 queens, got Q={Q}")
        p.n_queens = Q
    return p


def beta_values(schedule_params, n_steps):
    """beta(step) for step = 0 .. n_steps - 1 exactly as the reference evaluates it (experiments.py:13-77): the same NumPy
    functions on float64 in the same order, vectorised (NumPy's scalar and array exp / log / cos agree bit for bit).  This is
    what the sweep is given as mcq_params.beta_table, so that beta is the reference's own value and not a second math
    library's opinion of it."""
    st, bc, bs, be = _check_schedule(schedule_params)
    n = int(n_steps)
    step = np.arange(n, dtype=np.float64)
    if st == "constant":
        return np.full(n, float(bc), dtype=np.float64)
    if n <= 1:
        return np.full(n, float(be), dtype=np.float64)
    if st == "linear_annealing":
        frac = step / (n - 1)
        return bs + frac * (be - bs)
    if st == "exponential_annealing":
        log_ratio = np.log(be / bs)
        t = np.clip(step, 0, n - 1) / (n - 1)
        return bs * np.exp(log_ratio * t)
    if st == "logarithmic_annealing":
        log_norm = np.log(1 + n)
        return bs + (be - bs) * (np.log(1 + np.clip(step, 0, n)) / log_norm)
    x = (np.pi * np.clip(step, 0, n)) / n
    return bs + ((be - bs) * (1 - np.cos(x))) / 2


def beta_table(params, schedule_sets=None, schedule_params=None):
    """The [n_sets][n_steps] float64 table of a Params block (beta_values per schedule)."""
    sps = schedule_sets if schedule_sets is not None else [schedule_params]
    return np.ascontiguousarray(np.stack([beta_values(sp, params.n_steps) for sp in sps]).reshape(len(sps), int(params.n_steps)))


def seeds_for(base_seed, n_chains):
    """Chain r is seeded with base_seed + r (experiments.py:508); NumPy's legacy seed() accepts
    only 0 <= seed <= 2**32 - 1 and raises ValueError otherwise."""
    s = np.arange(n_chains, dtype=np.int64) + int(base_seed)
    if n_chains and (s[0] < 0 or s[-1] > 2**32 - 1):
        raise ValueError("Seed must be between 0 and 2**32 - 1")
    return s.astype(np.uint32)


def copy_params(params):
    """A private copy of a Params block (the schedule-set array it may point to is kept alive with the copy)."""
    p = Params.from_buffer_copy(params)
    keep = getattr(params, "_sets_keepalive", None)
    if keep is not None:
        p._sets_keepalive = keep
    for k in ("_schedules", "_beta_keepalive", "_ladder_keepalive", "_stream_keepalive"):
        if hasattr(params, k):
            setattr(p, k, getattr(params, k))
    return p


def host_beta_table(params):
    """float64 [n_sets][n_steps] of a Params built by make_params / make_params_sets, or None when the schedules are not
    known on the Python side (`_schedules` absent or None: a hand-filled struct -- the device then evaluates them itself).
    The values are derived from the struct's own fields (sched / beta_* and sets[t]), the ones the library would read, so a
    Params edited after make_params runs the schedule it now describes, not the one it was built with."""
    if not getattr(params, "_schedules", None) or params.n_steps <= 0:
        return None
    names = {v: k for k, v in SCHED.items()}

    def as_dict(s):
        if s.sched not in names:
            raise ValueError(f"Unknown betta_scheduling type: {s.sched}")
        return {"type": names[s.sched], "beta_const": float(s.beta_const), "beta_start": float(s.beta_start), "beta_end": float(s.beta_end)}

    sch = [as_dict(params.sets[t]) for t in range(int(params.n_sets))] if params.n_sets > 1 else [as_dict(params)]
    return np.ascontiguousarray(np.stack([beta_values(sp, params.n_steps) for sp in sch]))


def set_stream_states(params, states):
    """Chains that continue MT19937 streams instead of seeding them (include/mcq.h: stream_states; metropolis_mcmc(seed=None),
    experiments.py:200-201, 287-288): `states` is one np.random.get_state() tuple -- ('MT19937', key[624], pos, ...) -- per chain, or an
    array [n_chains][625] of key words + position.  Returns params."""
    if isinstance(states, np.ndarray):
        arr = np.ascontiguousarray(states, dtype=np.uint32)
    else:
        if isinstance(states, tuple) and len(states) >= 3 and isinstance(states[0], str):
            states = [states]
        rows = []
        for st in states:
            if st[0] != "MT19937":
                raise ValueError("only MT19937 states can be continued")
            rows.append(np.concatenate([np.asarray(st[1], dtype=np.uint32), np.array([int(st[2])], dtype=np.uint32)]))
        arr = np.ascontiguousarray(np.stack(rows))
    if arr.shape != (params.n_chains, 625):
        raise ValueError("one MT19937 state (624 key words + position) per chain")
    if (arr[:, 624] > 624).any():
        raise ValueError("MT19937 position out of range")
    params.stream_states = arr.ctypes.data
    params._stream_keepalive = arr
    return params


# include/mcq.h, exchange_ladder: the sweep's bracket works on the float32 image of a multiplier, so it must be a normal float32 number
LADDER_MIN, LADDER_MAX = float(np.finfo(np.float32).tiny), float(np.finfo(np.float32).max)
LADDER_RANGE_ERROR = "exchange_ladder entries must be finite and positive, within float32's normal range [2^-126, 2^127 (2 - 2^-23)]"


def set_exchange(params, every, ladder):
    """Turn on replica exchange (include/mcq.h: exchange_every / exchange_replicas / exchange_ladder) on a Params block:
    every `every` steps neighbouring rungs of each ladder of len(ladder) consecutive chains are offered a swap of their beta
    multipliers.  NOT a mode of the reference.  Returns params."""
    lad = np.ascontiguousarray(ladder, dtype=np.float64)
    if int(every) <= 0:
        raise ValueError("exchange_every must be positive")
    if lad.ndim != 1 or len(lad) not in (2, 4, 8, 16):
        raise ValueError("the exchange ladder has 2, 4, 8 or 16 rungs")
    if params.n_chains % len(lad) or (params.n_sets > 1 and params.chains_per_set % len(lad)):
        raise ValueError("n_chains (and chains_per_set) must be multiples of the number of rungs")
    if not np.all((lad >= LADDER_MIN) & (lad <= LADDER_MAX)):  # NaN fails both compares
        raise ValueError(LADDER_RANGE_ERROR)
    params.exchange_every, params.exchange_replicas = int(every), len(lad)
    params.exchange_ladder = lad.ctypes.data_as(C.POINTER(C.c_double))
    params._ladder_keepalive = lad
    return params


def make_resume(params, first_step, schedule_steps, state=None, stream_state=None):
    """A Resume block for a call with `params` (host buffers: _lib.run_host_from): steps [first_step, first_step + n_steps) of a
    schedule of `schedule_steps` steps, from `state` (uint8[n_chains][state_bytes], the final_state layout; None: the initial
    state) and `stream_state` (uint32[n_chains][625], np.random.get_state() key words + position; None: seeded)."""
    r = Resume()
    r.first_step, r.schedule_steps = int(first_step), int(schedule_steps)
    n, sb = int(params.n_chains), state_bytes(params.N, params.mode, params.n_queens)
    if state is not None:
        st = np.ascontiguousarray(state, dtype=np.uint8)
        if st.shape != (n, sb):
            raise ValueError(f"state must be uint8[{n}][{sb}] for these parameters, got {st.shape}")
        if st.ctypes.data % 16:  # rows are read 16 bytes at a time
            buf = np.zeros(st.size + 16, dtype=np.uint8)
            off = (-buf.ctypes.data) % 16
            al = buf[off: off + st.size].reshape(st.shape)
            al[...] = st
            st = al
            r._state_base = buf
        r.state = st.ctypes.data
        r._state_keepalive = st
    if stream_state is not None:
        ss = np.ascontiguousarray(stream_state, dtype=np.uint32)
        if ss.shape != (n, 625):
            raise ValueError("one MT19937 state (624 key words + position) per chain")
        r.stream = ss.ctypes.data
        r._stream_keepalive = ss
    return r


def segment_beta_table(params, first_step, schedule_steps):
    """float64 [n_sets][n_steps]: entries [first_step, first_step + n_steps) of the beta table of the WHOLE schedule of
    `schedule_steps` steps -- the reference's own arithmetic on the whole run (beta_values), sliced, so a run in segments gets the
    values the unbroken run gets.  None when the schedules are not known on the Python side (host_beta_table)."""
    if not getattr(params, "_schedules", None) or params.n_steps <= 0:
        return None
    whole = copy_params(params)
    whole.n_steps = int(schedule_steps)
    tab = host_beta_table(whole)
    a = int(first_step)
    return np.ascontiguousarray(tab[:, a: a + int(params.n_steps)])
