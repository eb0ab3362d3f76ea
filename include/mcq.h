/*
 * mcq.h -- C-ABI of the MI355X-native Metropolis sweep for the 3D N^2-queens problem.
 *
 * The reference (galgantar/monte-carlo-collective) has no FFI or plugin interface: its
 * seam is the Python function run_experiment() (experiments.py:475-573), which fans one
 * task per chain out to a process pool (experiments.py:507-517) and each task runs
 * metropolis_mcmc_board (experiments.py:282-376) or metropolis_mcmc
 * (experiments.py:199-279).  This header is the boundary a maintainer of the reference
 * would bind with ctypes to replace that fan-out + sweep: one call runs ALL chains.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes only; the library never returns owned memory.
 *   - every function returns 0 on success, a negative MCQ_E* code on error; the message
 *     for the last error of the calling thread is mcq_last_error().
 *   - no exceptions cross the boundary; the Python side maps MCQ_EINVAL to ValueError
 *     (the reference raises ValueError for unknown schedule / init modes:
 *     experiments.py:105, mcmc.py:104, mcmc_board.py:59) and the rest to RuntimeError.
 *
 * Two libraries export (subsets of) this interface:
 *   libmcq_hip.so     the product: hand-written HIP kernels for gfx950 (csrc/).
 *   libmcq_oracle.so  TEST INFRASTRUCTURE ONLY: a plain-C CPU restatement of the
 *                     reference algorithm (oracle/), exporting mcq_oracle_run().
 */
#ifndef MCQ_H
#define MCQ_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MCQ_ABI_VERSION 6

/* error codes */
#define MCQ_OK 0
#define MCQ_EINVAL (-1)   /* bad parameter (-> ValueError) */
#define MCQ_EDEVICE (-2)  /* HIP runtime error, no device, launch failure */
#define MCQ_ENOMEM (-3)   /* workspace too small / allocation failure */

/* mcmc_type: experiments.py:497-502 ("board" -> board chain, anything else -> full_3d) */
#define MCQ_MODE_BOARD 0
#define MCQ_MODE_FULL3D 1

/* init_mode: mcmc_board.py:26-59, mcmc.py:20-104 */
#define MCQ_INIT_RANDOM 0
#define MCQ_INIT_LATIN 1
#define MCQ_INIT_KLARNER 2

/* betta_scheduling.type: experiments.py:79-105 */
#define MCQ_SCHED_CONSTANT 0
#define MCQ_SCHED_LINEAR 1
#define MCQ_SCHED_EXPONENTIAL 2
#define MCQ_SCHED_LOGARITHMIC 3
#define MCQ_SCHED_SINUSOIDAL 4

/* random stream */
#define MCQ_RNG_MT19937_NUMPY 0 /* NumPy legacy global RandomState: bit-parity with the reference */
#define MCQ_RNG_PHILOX4X32_10 1 /* counter-based fast mode, NOT a stream of the reference: word w of chain r is
                                   philox4x32-10(counter = (low 32 bits of w / 4, high bits of w / 4, 0, 0), key = (seeds[r], 0))[w % 4], consumed with the same
                                   rules as the NumPy stream (masked rejection, 53-bit doubles, Fisher-Yates); no generator state
                                   lives in memory.  Results equal the oracle's in the same mode, not the reference's. */

/* energy_history trace */
#define MCQ_TRACE_NONE 0 /* only per-chain summaries (measure_min_energy_vs_N discards histories: experiments.py:1061) */
#define MCQ_TRACE_I32 1  /* full int32 trace + accept bits (experiments.py:355, 329-332) */
#define MCQ_TRACE_REDUCED 2 /* no per-chain trace: per-entry sums over the chains (what the plots consume, experiments.py:593-595, 660-695) */

/* flags */
#define MCQ_FLAG_EXACT_EXP 1u        /* evaluate exp(-beta*dE) in float64 on every step (disable the float32 bracket) */
#define MCQ_FLAG_SEQUENTIAL_DRAWS 2u /* HIP: draw every proposal word by word (disable the batched selection); for testing */
#define MCQ_FLAG_LINE_COUNTERS 4u    /* HIP: boards up to N = 8 at 4 lanes per chain take dE from per-line occupancy counters in LDS (one byte per line of
                                        the 12 families, 2 N^2 + 6 N (2N-1) + 4 (2N-1)^2 bytes per chain) instead of bit-mask probes of the heights; ignored
                                        where it does not apply (larger N, other lane counts, Philox, reduced trace, exchange).  Never changes a result. */
#define MCQ_FLAG_SHARED_PACING 16u   /* HIP: the launch paces its wavefronts (s_setprio by progress) against ALL launches of this process on the device that
                                        set the flag -- one progress table per device -- and does so whatever its size; without the flag a launch paces itself against
                                        its own wavefronts only, and only when it puts two or more on a SIMD.  For callers that run several launches of equal length
                                        side by side (jobs.JobSet).  Never changes a result. */
/* HIP: bits 8..9 of flags = the hardware priority (s_setprio 0..3) the launch's wavefronts run at when the launch is too small to pace
 * itself (fewer than two wavefronts per SIMD).  For callers that run several launches side by side: the long ones get precedence, the
 * short ones fill the gaps.  Never changes a result.  MCQ_FLAG_PRIORITY(p) builds the bits. */
#define MCQ_FLAG_PRIORITY_SHIFT 8
#define MCQ_FLAG_PRIORITY(p) (((uint32_t)(p) & 3u) << MCQ_FLAG_PRIORITY_SHIFT)

/* Upper bounds of this build (N >= 2 is required by the reference loop at experiments.py:317-319; the reference itself is
 * unbounded).  full_3d: column occupancy is one word per column -- 16 bits up to N = 16, 32 up to N = 32, 64 up to N = 64 (that variant:
 * 16 lanes per chain, NumPy's stream, no replica exchange; the queen table and the N^3 cells np.random.choice permutes live in the
 * workspace: N^3 * 4 bytes for each of the chains one round of the init kernel takes -- as many as 1 GiB holds).  board: bit masks up to N = 32, a compare per probed
 * height beyond (slower, any size whose N*N heights fit a wavefront's share of the LDS and whose accept flags fit a byte). */
#define MCQ_MIN_N 2
#define MCQ_MAX_N 64        /* mcmc_type full_3d (beyond 32: 64-bit column words, 16 lanes per chain) */
#define MCQ_MAX_N_BOARD 128 /* mcmc_type board */

/* One set of a batched run: its beta schedule (run_beta_start_end_pairs loops over such pairs: experiments.py:741-846) and,
 * optionally, its own init mode. */
typedef struct mcq_schedule {
    int32_t sched;     /* MCQ_SCHED_* */
    int32_t init_plus1; /* 0: the set starts from mcq_params.init; otherwise MCQ_INIT_* + 1 -- the (init_mode, N) cells of
                           measure_min_energy_vs_N that share N (experiments.py:1050-1067) then run as one launch */
    double beta_const;
    double beta_start;
    double beta_end;
} mcq_schedule;

typedef struct mcq_params {
    int32_t abi_version;     /* MCQ_ABI_VERSION */
    int32_t N;               /* board edge; Q = N*N queens */
    int32_t mode;            /* MCQ_MODE_* */
    int32_t init;            /* MCQ_INIT_* */
    int32_t sched;           /* MCQ_SCHED_* */
    int32_t rng;             /* MCQ_RNG_* */
    int32_t trace;           /* MCQ_TRACE_* */
    uint32_t flags;          /* MCQ_FLAG_* */
    double beta_const;       /* constant schedule            (experiments.py:13-16)  */
    double beta_start;       /* annealing schedules          (experiments.py:19-77)  */
    double beta_end;
    int64_t n_steps;         /* steps per chain = schedule length                    */
    int64_t n_chains;        /* n_runs (< 2^31); chain r is seeded with seeds[r] (= base_seed + r, experiments.py:508) */
    int64_t patience;        /* early_stop_patience, board only (experiments.py:349-353); < 0 = None */
    int64_t hist_stride;     /* int32 elements per chain row of energy_hist, >= n_steps + 1, a multiple of 16 and < 2^24 (HIP: rows
                                are written in aligned 64-byte segments; energy_hist itself must be 64-byte aligned; runs of more
                                than 2^24 - 16 steps take trace = REDUCED or NONE) */
    int64_t bits_stride;     /* uint64 words per chain row of accept_bits, >= ceil(n_steps / 64) */
    int32_t lanes_per_chain; /* HIP only: 2 (boards), 4, 8 or 16 lanes of a wavefront per chain; 0 = library default */
    int32_t device;          /* HIP only, host-buffer entry point: device ordinal, < 0 = current device */
    /* Several schedules in ONE launch (everything else shared): n_sets <= 1 means the single schedule above.  Otherwise
     * chains [t * chains_per_set, (t + 1) * chains_per_set) follow sets[t]; n_chains == n_sets * chains_per_set,
     * chains_per_set is a multiple of 16, and with trace == REDUCED the step_* outputs are [n_sets][n_steps + 1]. */
    int64_t n_sets;
    int64_t chains_per_set;
    const mcq_schedule* sets; /* HOST pointer (also for mcq_run_device), n_sets entries */
    /* Optional beta(step) values, double[n_sets <= 1 ? 1 : n_sets][n_steps] (set-major): when given, the sweep uses exactly
     * these instead of evaluating the schedule on the device.  The reference evaluates its schedules with NumPy's exp / log /
     * cos (experiments.py:27-77), whose last bit differs between NumPy, glibc and the GPU's math library on ~0.1-5 % of the
     * arguments; a caller that wants beta bit-identical to the reference passes the reference's own values (the Python side
     * does: abi.host_beta_table).  mcq_run_device: DEVICE pointer; mcq_run_host: HOST pointer.  NULL: computed on the device
     * (exact for constant / linear; the other three within 2^-51 * max(|beta_start|, |beta_end|) of the reference's value). */
    const double* beta_table;
    /* Replica exchange (parallel tempering) between the chains of a launch -- NOT a mode of the reference (its report, section VI,
     * names better moves as future work), never a default, results equal the oracle's in the same mode.
     * exchange_every = K > 0 turns it on: chains [g * R, (g + 1) * R), R = exchange_replicas (2, 4, 8 or 16; n_chains and
     * chains_per_set are multiples of R), form one ladder.  Chain r starts on rung r % R; a chain on rung t runs every step s
     * at beta(s) * exchange_ladder[t] (one float64 multiply; beta(s) from the schedule / beta_table as without exchange).
     * After every K-th step (steps K-1, 2K-1, ... of the run, n = (s + 1) / K = 1, 2, ...) the rungs (t, t + 1) with
     * t = (n & 1), (n & 1) + 2, ... <= R - 2 are offered a swap: with a, b the chains on rungs t, t + 1,
     *     x = (beta_a - beta_b) * (double)(E_a - E_b),   beta_a = beta(s) * ladder[t],  beta_b = beta(s) * ladder[t + 1],
     * the chain on rung t draws u = random() from ITS stream (two words, right after its step-s words; always drawn) and the two
     * chains trade rungs iff u < min(1, exp(x)) -- the reference's accept rule (experiments.py:326-327) on the pair.  States,
     * energies and histories stay with their chains; only the rung (hence beta) moves.  Needs patience < 0 (no early stop) and
     * trace != REDUCED. */
    int64_t exchange_every;        /* 0 = off */
    int32_t exchange_replicas;     /* R */
    int32_t n_queens;              /* full_3d only: Q queens instead of N*N (State3DQueens(N, Q=...), mcmc.py:6-18; metropolis_mcmc(..., Q=...),
                                      experiments.py:199-203), 2 <= Q < N^3, random init only (latin / klarner assume Q = N^2: mcmc.py:21-25);
                                      0 = N*N.  state_bytes becomes 3 Q (mcq_state_bytes_for). */
    const double* exchange_ladder; /* HOST pointer (also for mcq_run_device), R positive multipliers, each within float32's normal range
                                      [2^-126, 2^127 (2 - 2^-23)]: the sweep's float32 bracket of the accept test runs at (float)ladder[t], which
                                      must be neither 0 nor infinity; anything else is MCQ_EINVAL, in the oracle too.  What remains: under exchange
                                      a |beta(step)| beyond float32's range is followed through its float32 image (0 or infinity) in the bracket,
                                      where beta(step) * ladder[t] may still be an ordinary number; without exchange there is no such limit (a beta
                                      whose image is 0 or infinity has exp(-beta dE) = 1 or 0 in float64 as well).  Read during the call: validated, and copied to the
                                      device with a hipMemcpyAsync on the caller's stream from THIS (normally pageable) array, so it must stay valid until
                                      that copy has run -- mcq_run_host and the Python wrappers keep it alive and synchronise; a caller of mcq_run_device
                                      keeps it until the stream has passed the call (with exchange the call cannot be part of a stream capture) */
    /* Chains that CONTINUE a random stream instead of seeding one: metropolis_mcmc[_board](..., seed=None) skips np.random.seed and draws from
     * NumPy's global RandomState wherever it stands (experiments.py:200-201, 287-288).  Optional, uint32[n_chains][625]: per chain the 624 key
     * words and the position (0..624) of an MT19937 state exactly as np.random.get_state() returns them; seeds[r] is ignored for such a run.
     * HOST pointer (also for mcq_run_device: the library rewinds the unconsumed part of the generation into the layout its kernels stream from,
     * copies the states to the workspace and synchronises the stream once); MCQ_RNG_MT19937_NUMPY only.  mcq_outputs.stream_words tells how far
     * each chain went, so the caller can advance its own copy of the stream by as many words. */
    const uint32_t* stream_states;
} mcq_params;

/*
 * Per-chain outputs; every array is caller-allocated.  state_bytes = mcq_state_bytes(N, mode) (mcq_state_bytes_for(p) with n_queens):
 *   board:   N*N uint8 heights, row-major heights[i][j]        (mcmc_board.py:28)
 *   full_3d: Q*3 uint8 (i, j, k) per queen, in queen-index order (mcmc.py:101)
 * Pointers that may be NULL are marked optional.
 */
typedef struct mcq_outputs {
    int32_t* energy_hist;    /* optional unless trace == I32: [n_chains][hist_stride]; entry 0 = E0, entry s+1 = energy after step s */
    uint64_t* accept_bits;   /* optional unless trace == I32: [n_chains][bits_stride]; bit (s & 63) of word s >> 6 = step s accepted */
    int64_t* hist_len;       /* [n_chains] entries of energy_hist that are valid (n_steps + 1, fewer after an early stop) */
    int64_t* steps_executed; /* [n_chains] proposals made (hist_len - 1, +1 when the chain broke out early) */
    int32_t* initial_energy; /* [n_chains] E0 */
    int32_t* best_energy;    /* [n_chains] */
    int32_t* final_energy;   /* [n_chains] */
    int64_t* steps_to_best;  /* [n_chains] first index of min(energy_history) (experiments.py:364-365) */
    int64_t* n_accepted;     /* [n_chains] */
    int64_t* near_ties;      /* optional [n_chains]: steps whose uniform fell within 4 ulp of the acceptance probability */
    uint8_t* best_state;     /* optional [n_chains][state_bytes]; HIP: 16-byte aligned base (rows are copied 16 bytes at a time) */
    uint8_t* final_state;    /* optional [n_chains][state_bytes]; HIP: 16-byte aligned base */
    /* trace == REDUCED only, int64[n_steps + 1] each (per schedule set: [n_sets][n_steps + 1]), indexed by history entry e
     * (entry 0 = initial state): */
    int64_t* step_sum;       /* sum over chains of energy_history[e]                                   */
    int64_t* step_sumsq;     /* sum of squares                                                         */
    int64_t* step_accepted;  /* chains whose step e - 1 was accepted (entry 0: 0); includes the step at which a chain stopped
                                early, which is executed and listed in accepted_steps but appends no entry (experiments.py:329-353) */
    int64_t* step_count;     /* chains whose history has entry e (< n_chains only after early stops)    */
    /* exchange_every > 0 only, optional [n_chains] each: */
    int32_t* exchange_rung;  /* the rung the chain ends on */
    int64_t* n_exchanges;    /* accepted swaps the chain took part in */
    uint32_t* stream_words;  /* optional [n_chains]: 32-bit words the chain took from its random stream -- initial state, every step's draws (the
                                rejected words of randint included), exchange uniforms -- modulo 2^32; 0 with MCQ_RNG_PHILOX4X32_10 (a stream addressed
                                by position: nothing to hand back).  Equal between the oracle and the kernels like every other output: the streams
                                are consumed identically, not only the results */
} mcq_outputs;

/* ---- exported by libmcq_hip.so ------------------------------------------------------------ */

int mcq_abi_version(void);
const char* mcq_last_error(void);
int mcq_device_count(void);

/* lanes of a wavefront per chain used when mcq_params.lanes_per_chain == 0: board 4 up to N = 12 and 8 beyond, full_3d 8 (16 beyond
 * N = 32, the only width of that variant; 4 for N = 9..12 with NumPy's stream) (mcq_default_lanes: the value for small boards).  A board launch that leaves SIMDs empty runs at twice or four times the
 * lanes while every wavefront still has a SIMD to itself (N >= 20: at most 8; N <= 8: always 4); with replica exchange a ladder must fit one
 * wavefront.  mcq_effective_lanes tells.  The lane count never changes a result. */
/* mcq_params.stream_states, one chain: an MT19937 state as np.random.get_state() holds it (uint32[625]: key, position) in the layout the kernels stream
 * from (uint32[626]: words [0, out[625]) of the current generation, the rest rewound to the generation before; out[624] = position).  Pure host code:
 * what mcq_run_device does with every state before it copies them to the workspace; exported for the tests. */
void mcq_stream_layout(const uint32_t* numpy_state, uint32_t* out);
int32_t mcq_default_lanes(int32_t mode);
int32_t mcq_default_lanes_n(int32_t mode, int32_t N);
/* the lane count a launch with these parameters really runs with (lanes_per_chain, or the default above and its small-launch
 * rule, which looks at the current device); 0 on bad arguments */
int32_t mcq_effective_lanes(const mcq_params* p);
/* SIMDs of the current device (4 per compute unit; 1024 when no device answers): what the small-launch rule compares with */
int32_t mcq_device_simds(void);
/* Inspection: the instantiation of the sweep kernel a launch with these parameters takes on the current device.  variant[13]: the
 * kernel's template arguments in their order -- MODE, G (= mcq_effective_lanes), PATIENCE, NT, REDUCED, PHILOX, NC, EXCH, CAND5,
 * EARLYU, SLIM, CNT, WIDE (bools as 0 / 1) --, *lds_bytes: the dynamic LDS of a workgroup (one wavefront).  Pure host code: it looks
 * at the device's SIMD count only (1024 when no device answers).  Every variant gives the same results; this exists so that the
 * choice, which only speed depends on, can be tested.  Returns what mcq_run_device would refuse these parameters with before it
 * enqueues anything (bad arguments, a lane count the mode does not run, a chain state beyond the LDS), the text in mcq_last_error. */
int mcq_sweep_variant(const mcq_params* p, int32_t variant[13], int64_t* lds_bytes);

/* bytes of one chain's state record in best_state / final_state; 0 on bad arguments.  mcq_state_bytes: Q = N*N queens;
 * mcq_state_bytes_for: the parameter block's own count (n_queens). */
size_t mcq_state_bytes(int32_t N, int32_t mode);
size_t mcq_state_bytes_for(const mcq_params* p);

/* bytes of device scratch mcq_run_device needs for these parameters; 0 on bad arguments */
size_t mcq_workspace_bytes(const mcq_params* p);

/*
 * Replaces run_experiment's fan-out + per-chain sweep (experiments.py:507-546) with
 * device-resident buffers.  `seeds` (uint32[n_chains]) and every non-NULL pointer of
 * `out` are DEVICE pointers; `workspace` is a 64-byte aligned device buffer of at least
 * mcq_workspace_bytes(p) bytes (hipMalloc results are).  Violations return MCQ_EINVAL.  Work is enqueued on `hip_stream` (a hipStream_t, NULL =
 * the default stream) and the call returns without synchronising.
 */
int mcq_run_device(const mcq_params* p, const uint32_t* seeds, const mcq_outputs* out,
                   void* workspace, size_t workspace_bytes, void* hip_stream);

/*
 * mcq_run_device plus HIP events recorded on `hip_stream` around the init kernel and around the
 * sweep kernel; waits for the last event and returns both device times in milliseconds.  Blocking.
 */
int mcq_run_device_timed(const mcq_params* p, const uint32_t* seeds, const mcq_outputs* out, void* workspace,
                         size_t workspace_bytes, void* hip_stream, float* init_ms, float* sweep_ms);

/*
 * Statistics of a device-resident trace (what plot_energy_histories, experiments.py:593-595, and
 * plot_acceptance_rates_binned, experiments.py:660-695, consume), so that the trace never crosses PCIe.
 * `out` holds the DEVICE buffers a previous mcq_run_device filled.  All result arrays are device pointers:
 *   step_sum / step_sumsq / step_count  int64[n_steps + 1]: over the chains whose history reaches that entry
 *                                       (count < n_chains only after early stops); pass NULL to skip
 *   bin_lo  int64[n_bins + 1]: first step of every bin (ascending, bin_lo[n_bins] >= n_steps closes the last);
 *   bin_accepted / bin_proposed uint64[n_bins]: accepted / executed steps of all chains per bin; n_bins = 0 to skip
 * Enqueued on `hip_stream`; asynchronous.
 */
int mcq_trace_stats_device(const mcq_params* p, const mcq_outputs* out, int64_t* step_sum, int64_t* step_sumsq,
                           int64_t* step_count, int32_t n_bins, const int64_t* bin_lo, uint64_t* bin_accepted,
                           uint64_t* bin_proposed, void* hip_stream);

/*
 * The node-level summary of a finished launch, packed for the ONE all-reduce of a job list (the layout of the host side's
 * distributed.py): replaces the per-run gathering of run_experiment (experiments.py:519-546) and the statistics the drivers take from it
 * (experiments.py:1074-1096) with one or two small kernels per launch, where the host side needed ~10 tensor operations per job.
 * One mcq_pack_slot per schedule set of the launch (n_sets <= 1: one) says where that job's fields sit in `packed` (word offsets; -1 = absent).
 * The set's chains on this rank are [t * chains_per_set, t * chains_per_set + n_local).  `packed` must have been zeroed; the call WRITES the
 * counters and slots of its jobs (other ranks' shares arrive by the all-reduce) and adds to the stopped-chain histogram.
 * `out` holds the DEVICE buffers mcq_run_device filled (hist_len, steps_executed, best_energy, steps_to_best, n_accepted; with a stats offset
 * the four step_* arrays of trace == REDUCED).  Enqueued on `hip_stream`; asynchronous.
 */
typedef struct mcq_pack_slot {
    int64_t counters; /* 6 words: chains, accepted, proposed, sum of best_energy, sum of its squares, sum of steps_to_best */
    int64_t min_slot; /* this rank's slot of the per-rank minima: min(best_energy) + 1 (0 = the rank holds no chain of the job) */
    int64_t best;     /* first of the n_local per-chain slots of best_energy (already offset to this rank's first chain), or -1 */
    int64_t stb;      /* the same for steps_to_best, or -1 */
    int64_t stats;    /* first of 5 x (n_steps + 1) words: per-entry sum, sum of squares, accepted, count, chains that stopped early at the entry; or -1 */
} mcq_pack_slot;
int mcq_pack_summary_device(const mcq_params* p, const mcq_outputs* out, int64_t n_local, const mcq_pack_slot* slots /* HOST, one per set */,
                            int64_t* packed /* DEVICE */, void* hip_stream);

/*
 * The beta(step) table the sweep reads (experiments.py:13-77 evaluated on the device in float64, strict IEEE):
 * `beta_out` is a DEVICE buffer of double[n_sets][n_steps] (n_sets <= 1: [n_steps]); `c32_out` (optional, DEVICE,
 * float, same shape) receives (float)(-beta * log2(e)), the factor of the float32 accept bracket.  Inspection /
 * testing only: mcq_run_device computes its own tables.  Enqueued on `hip_stream`; asynchronous.
 */
int mcq_beta_table_device(const mcq_params* p, double* beta_out, float* c32_out, void* hip_stream);

/*
 * Same computation with HOST buffers: allocates device memory, uploads seeds, runs,
 * downloads every non-NULL output and frees.  Blocking.  `kernel_seconds` (optional)
 * receives the device time of init + sweep measured with HIP events.
 */
int mcq_run_host(const mcq_params* p, const uint32_t* seeds, const mcq_outputs* out,
                 double* kernel_seconds);

/*
 * Chains that go on where an earlier call left them (ABI 6).  mcq_run_device and mcq_run_host are one shot: seed, build the initial state,
 * sweep n_steps.  The *_from calls run steps [first_step, first_step + p->n_steps) of a schedule of schedule_steps steps, from the initial
 * state (a first segment) or from given placements and MT19937 states; mcq_checkpoint_device hands the streams back.  Run [0, K) with
 * state = NULL, checkpoint, run [K, T) from the checkpoint (state = the first call's final_state, stream = the checkpoint's states): the
 * two energy histories (entry 0 of the second repeats the last entry of the first), accept bits, final state and stream equal those of ONE
 * mcq_run_device with n_steps = T word for word, for any K and any number of cuts.
 *   - beta of step s of the call is beta(first_step + s) of the schedule_steps-long schedule.  A p->beta_table covers THIS call's n_steps
 *     (the caller slices the whole table); without one the device evaluates the schedule with the offset and the whole length.
 *   - every output is relative to the call: initial_energy (recounted from the given state, so it can be checked against the final_energy
 *     of the call before), best_energy, steps_to_best, n_accepted, stream_words, the step_* arrays of the reduced trace.  Merging the
 *     segments is host work (monte-carlo-collective_amd/checkpoint.py).
 *   - with `state` given, p->init and sets[].init_plus1 are ignored and no initialisation draw is taken.
 *   - schedule sets, every trace mode, lane count and size mcq_run_device serves are served.
 * MCQ_EINVAL (mcq_validate_resume tells without a device): first_step < 0 or first_step + n_steps > schedule_steps; exchange_every > 0 (the
 * rungs are not part of a checkpoint); a board patience that could trigger, 0 <= patience <= schedule_steps (the no-improvement counter is
 * not carried); rng = PHILOX with `stream` or `state`; `stream` without `state` (a first segment that continues a stream takes
 * p->stream_states); `state` with p->stream_states; a `state` that is not 16-byte aligned.
 * NOT checked, the data being on the device -- it is made harmless instead: a position above 624 in `stream` reads as 624, and every byte of
 * `state` is clamped to N - 1 (a board height or a full_3d coordinate beyond the board); two queens of a full_3d state on one cell share a
 * column bit, so the energies of such a chain mean nothing, and nothing outside the chain's own tables is touched.
 * `state` may be out->final_state of the same call (the usual chain of segments): the placements are read by the kernel that takes the
 * init kernel's place, which has finished before the sweep writes final_state.
 * A `stream` at position 0 (NumPy never stands there by itself: only set_state() puts it there) is continued like any other, but the low
 * 31 bits of key word 0 that a checkpoint hands back BEFORE the chain has drawn its first generation are not the caller's: no twist ever
 * reads those bits, so every draw is the same; only the comparison of that one key word with the caller's copy is not.
 */
typedef struct mcq_resume {
    int64_t first_step;     /* index, in the WHOLE schedule, of this call's step 0 */
    int64_t schedule_steps; /* length of the whole schedule; the call runs steps [first_step, first_step + p->n_steps) of it */
    const uint8_t* state;   /* [n_chains][state_bytes], final_state layout, 16-byte aligned; NULL = build the initial state as mcq_run_device does
                               (first segment) */
    const uint32_t* stream; /* [n_chains][625] MT19937 states exactly as np.random.get_state() holds them (624 key words, position); NULL = seed
                               from seeds[r] (np.random.seed), taking no initialisation draws when `state` is given */
} mcq_resume;

/* the MCQ_EINVAL conditions above, pure host code: MCQ_OK or MCQ_EINVAL with mcq_last_error() */
int mcq_validate_resume(const mcq_params* p, const mcq_resume* from);

/* mcq_run_device for a segment: `from->state` / `from->stream` are DEVICE pointers, read by a kernel that takes the init kernel's place
 * (no host staging, no synchronise); asynchronous like mcq_run_device, same workspace (mcq_workspace_bytes(p)). */
int mcq_run_device_from(const mcq_params* p, const mcq_resume* from, const uint32_t* seeds, const mcq_outputs* out,
                        void* workspace, size_t workspace_bytes, void* hip_stream);
/* ... with the events of mcq_run_device_timed: init_ms is the restore kernel's time when `from->state` is given.  Blocking. */
int mcq_run_device_from_timed(const mcq_params* p, const mcq_resume* from, const uint32_t* seeds, const mcq_outputs* out, void* workspace,
                              size_t workspace_bytes, void* hip_stream, float* init_ms, float* sweep_ms);

/* Enqueued behind a run (mcq_run_device or mcq_run_device_from, MCQ_RNG_MT19937_NUMPY) on the same stream, with that run's parameters and
 * workspace: turns what the sweep left in the workspace into the MT19937 state NumPy itself would hold after as many draws -- one
 * generation, position 1 .. 624 (a chain that has consumed a whole generation reports 624, never 0) -- into `stream_out`, DEVICE
 * uint32[n_chains][625].  The placement half of a checkpoint is out->final_state of the run.  The workspace must not have been used in
 * between.  After a plain mcq_run_device the stream is where the chain left it, whatever made it leave: a board chain that stopped early
 * (patience) stands behind the words of its last executed step, and with replica exchange the exchange uniforms are counted like every
 * other word -- in both cases NumPy's state after out->stream_words words (such a run cannot be CONTINUED: mcq_validate_resume).  MCQ_EINVAL: rng = PHILOX; p->n_steps above 2^28 (the workspace counts the words of the segment in 32 bits).  Asynchronous. */
int mcq_checkpoint_device(const mcq_params* p, const mcq_outputs* out, void* workspace, size_t workspace_bytes, uint32_t* stream_out,
                          void* hip_stream);

/* mcq_run_host for a segment: `from->state`, `from->stream` and `stream_out` (optional: the checkpoint's states, uint32[n_chains][625])
 * are HOST buffers.  Blocking. */
int mcq_run_host_from(const mcq_params* p, const mcq_resume* from, const uint32_t* seeds, const mcq_outputs* out, uint32_t* stream_out,
                      double* kernel_seconds);

/*
 * Population annealing: the chains of a population are RESAMPLED between two segments (csrc/mcq_population.hip) -- NOT a mode of the
 * reference, never a default, like Philox and replica exchange.  A run of n_steps steps is cut into segments of S steps
 * (mcq_run_device_from); at boundary k = 1 .. K - 1 (K = ceil(n_steps / S)), before the segment that starts at step k S, slot m of a
 * population of R chains [g R, (g + 1) R) takes the PLACEMENT (and with it the energy) of a parent p(m) of the same population.  The
 * slot keeps its own random stream, its own history and its own running best.  The rule is integer-exact:
 *   1. dbeta_k = beta(k S) - beta((k - 1) S) >= 0, beta as the sweep reads it (float64, the reference's arithmetic).
 *   2. the caller's weight table T_k[d] = floor(2^24 exp(-dbeta_k d)) as uint32, d = 0 .. D - 1; D = 1 + the first d with T = 0, at most
 *      2^16.  T_k[0] = 2^24.
 *   3. E_r = the segment's final_energy, E_min = the population's minimum, d_r = min(E_r - E_min, D - 1), w_r = T_k[d_r];
 *      C_r = w_0 + .. + w_r (uint64, slot order), W = C_{R-1}.  R <= 2^19, so that R W < 2^64.
 *   4. one 32-bit offset word x per (boundary, population): U = floor(x W / 2^32) < W, from the full product.
 *   5. systematic resampling: p(m) = the smallest r with C_r R > m W + U.
 *   6. so chain r gets floor(R w_r / W) or ceil(R w_r / W) children, the map m -> p(m) is monotone, and equal weights (dbeta = 0) give
 *      the identity.
 * mcq_resample describes ONE boundary.  mcq_resample_device enqueues a few small kernels on the stream: the plan (per population:
 * min-reduce, table lookup and 64-bit prefix sum in one workgroup, then the search for p(m) with one lane per slot), the row gather
 * state_out[m] = state_in[parent[m]] -- which cannot run in place: two buffers --, and the per-slot fold of the finished segment's
 * summary into the run's.  The fold follows the merge rule of
 * chains in segments: a segment moves best_energy / best_state / steps_to_best (in whole-run steps: first_step + the segment's) only by
 * a STRICTLY lower energy; n_accepted, near_ties and stream_words (modulo 2^32) add up; first_step == 0 (the first segment) copies.
 * With state_in == NULL nothing is resampled and only the fold runs (the last segment of a run).
 */
#define MCQ_MAX_POPULATION (1 << 19)
#define MCQ_MAX_RESAMPLE_TABLE (1 << 16)
#define MCQ_RESAMPLE_WEIGHT_BITS 24

typedef struct mcq_resample {
    int64_t n_chains;          /* a multiple of population */
    int64_t population;        /* R: a multiple of 16, <= MCQ_MAX_POPULATION */
    int64_t state_bytes;       /* bytes of one placement row (mcq_state_bytes_for) */
    const uint32_t* table;     /* T_k, table_len entries */
    int64_t table_len;         /* D, 1 .. MCQ_MAX_RESAMPLE_TABLE */
    const uint32_t* offsets;   /* x, one word per population */
    const int32_t* energies;   /* [n_chains] final_energy of the finished segment */
    const uint8_t* state_in;   /* [n_chains][state_bytes] its final_state; NULL = fold only.  16-byte aligned when state_bytes % 16 == 0 */
    uint8_t* state_out;        /* [n_chains][state_bytes], not state_in; aligned like state_in */
    int32_t* parent;           /* [n_chains] p(m) as a chain index of the launch (g R + r) */
    int64_t* stats;            /* [n_chains / population][3]: distinct parents, W, E_min */
    int32_t* energy_out;       /* optional [n_chains]: energies[parent[m]] (not `energies`) */
    /* optional fold of the segment's per-slot summary (seg_*, what the segment's mcq_outputs hold) into the run's (run_*);
     * on when run_best_energy is given, then seg_best_energy, seg_steps_to_best, seg_n_accepted and the matching run_* are required */
    int64_t first_step;        /* index, in the whole schedule, of the finished segment's step 0 */
    const int32_t* seg_best_energy;
    const int64_t* seg_steps_to_best;
    const int64_t* seg_n_accepted;
    const int64_t* seg_near_ties;     /* optional, with run_near_ties */
    const uint32_t* seg_stream_words; /* optional, with run_stream_words */
    const uint8_t* seg_best_state;    /* optional, with run_best_state; rows of state_bytes, aligned like state_in */
    int32_t* run_best_energy;
    int64_t* run_steps_to_best;
    int64_t* run_n_accepted;
    int64_t* run_near_ties;
    uint32_t* run_stream_words;
    uint8_t* run_best_state;
} mcq_resample;

/* the message of the last error of the calling thread from the three mcq_resample_* calls below (they do not set mcq_last_error()) */
const char* mcq_population_last_error(void);
/* bytes of device scratch mcq_resample_device needs (the prefix sums C_r); 0 on bad arguments */
size_t mcq_resample_scratch_bytes(const mcq_resample* r);
/* One boundary on the device: every pointer of `r` and `scratch` (8-byte aligned) are DEVICE pointers.  Enqueued on `hip_stream`;
 * asynchronous, nothing is copied to the host.  MCQ_EINVAL: a population that is no multiple of 16, exceeds MCQ_MAX_POPULATION or does
 * not divide n_chains; table_len out of range; a missing pointer; misaligned rows; state_out == state_in.  NOT checked, being on the
 * device: a table with T[0] = 0 gives W = 0 and every slot of the population the parent g R + R - 1; nothing leaves the arrays. */
int mcq_resample_device(const mcq_resample* r, void* scratch, size_t scratch_bytes, void* hip_stream);
/* The plan alone -- steps 3 to 5 -- in pure host code: table, offsets, energies, parent and stats are HOST pointers, the rest of `r`
 * is ignored.  Equal to the plan kernel bit for bit; exported for the tests the way mcq_stream_layout is. */
int mcq_resample_plan_host(const mcq_resample* r);

/*
 * Quench: the deterministic zero-temperature descent of board placements to a local minimum under single-height moves
 * (csrc/mcq_quench.hip) -- NOT a mode of the reference, which ships the ingredient (State3DQueensBoard.conflicts_for_position,
 * mcmc_board.py:147-193) and never uses it; never a default.  It certifies a placement as a local minimum, recounts its energy on the
 * device independently of the sweep, and hands back the per-column conflict map.  Boards only.  The rule is integer-exact:
 *   1. every input byte is clamped to N - 1 first (as the restore kernel of mcq_run_device_from does).
 *   2. for a board of heights h[i][j], a column c = (i, j) and a height k, a(c, k) = the number of OTHER columns c' = (i', j') with
 *        di = 0 or dj = 0 or |di| = |dj|     (di = i' - i, dj = j' - j: same row, same column or a diagonal of the board), and
 *        |h(c') - k| = 0 or d,  d = max(|di|, |dj|)
 *      -- conflicts_for_position(i, j, k).  The energy is E = 1/2 sum_c a(c, h(c)) (_compute_energy, mcmc_board.py:82-122).
 *   3. one PASS visits the columns in row-major order.  For column c: k* = the SMALLEST k in 0 .. N - 1 with minimal a(c, k); if
 *      a(c, k*) < a(c, h(c)) then h(c) = k*, E += a(c, k*) - a(c, h(c)), and one move is counted.  Later columns of the same pass see
 *      the new height.
 *   4. passes repeat until one makes no move (the placement is then a local minimum: no single column has a height with a lower
 *      count) or max_passes passes have run (0 = no limit).  E falls by at least 1 per moving pass, so a run ends within
 *      energy_in + 1 passes; n_passes counts the last, moveless pass too (a local minimum comes back with n_moves = 0, n_passes = 1).
 * Chains do not interact, so state_out may be state_in.
 */
typedef struct mcq_quench {
    int32_t N;            /* MCQ_MIN_N .. MCQ_MAX_N_BOARD */
    int32_t mode;         /* MCQ_MODE_BOARD; full_3d is MCQ_EINVAL (a queen there has N^3 targets: a different design) */
    int64_t n_chains;     /* 1 .. 2^31 - 1 */
    int64_t max_passes;   /* >= 0; 0 = until a pass makes no move */
    const uint8_t* state_in; /* [n_chains][N*N], final_state layout */
    uint8_t* state_out;   /* [n_chains][N*N]; may be state_in */
    int32_t* energy_in;   /* optional [n_chains]: E of the (clamped) input, recounted */
    int32_t* energy_out;  /* optional [n_chains]: E of the output = energy_in + the sum of the moves' differences */
    int32_t* n_moves;     /* optional [n_chains] */
    int32_t* n_passes;    /* optional [n_chains] */
    uint16_t* conflicts;  /* optional [n_chains][N*N]: a(c, h(c)) of the OUTPUT placement; its sum is 2 energy_out */
} mcq_quench;

/* the message of the last error of the calling thread from the two mcq_quench_* calls below (they do not set mcq_last_error()) */
const char* mcq_quench_last_error(void);
/* Every pointer of `q` is a DEVICE pointer.  One kernel enqueued on `hip_stream`; asynchronous: nothing is copied back and nothing
 * synchronises.  MCQ_EINVAL before any launch: mode other than board, N out of range, n_chains outside 1 .. 2^31 - 1, a negative
 * max_passes, a NULL state_in or state_out. */
int mcq_quench_device(const mcq_quench* q, void* hip_stream);
/* The same rule in plain host code over HOST buffers, same refusals; needs no GPU.  Equal to the kernel bit for bit on every output;
 * exported for the tests the way mcq_resample_plan_host is. */
int mcq_quench_host(const mcq_quench* q);

/*
 * Heat-bath column sweeps of board placements (csrc/mcq_heatbath.hip) -- NOT a mode of the reference, whose only move is one random
 * column, one random height and one Metropolis test (its report lists better moves as future work); never a default, like Philox,
 * replica exchange, population annealing and the quench.  A column's new height is DRAWN from the Boltzmann weights of all N heights
 * at once, so no proposal is rejected.  Boards only.  The rule is integer-exact:
 *   1. every input byte is clamped to N - 1 first; a(c, k) and E are those of the quench rule above, items 1 - 2.
 *   2. a call runs n_sweeps sweeps; sweep s of the call has the global index g = first_sweep + s and visits the columns
 *      c = 0 .. N^2 - 1 in row-major order.  Later columns see earlier updates.
 *   3. for column c: a_min = min_k a(c, k); w_k = T_s[min(a(c, k) - a_min, D - 1)], T_s = the caller's row for sweep s (uint32,
 *      D = table_len entries, 1 <= D <= MCQ_MAX_HEATBATH_TABLE); C_k = w_0 + .. + w_k in uint32 (k = 0 .. N - 1), W = C_{N-1}.
 *      The Python side builds T_s[d] = floor(2^24 exp(-beta_s d)) in float64 with NumPy, beta_s >= 0, so T_s[0] = 2^24 and
 *      W <= 128 * 2^24 = 2^31; D = 1 + the first d with T = 0 over the call's rows, at most 512, rows zero-padded.  A caller's own
 *      table is as good, and every entry of T is at most 2^MCQ_HEATBATH_WEIGHT_BITS = 2^24: W then stays below 2^32 at N = 128, so
 *      the uint32 sums do not wrap and C is non-decreasing.
 *   4. one 32-bit word x per (chain, sweep, column): word w = g N^2 + c (64-bit) of chain r is
 *      philox4x32-10(counter = (low 32 bits of w / 4, high bits of w / 4, 0, 0), key = (seeds[r], 1))[w % 4] -- the definition of
 *      MCQ_RNG_PHILOX4X32_10 with key word 1 instead of 0, so the two streams are independent.  The state of a chain is its placement
 *      plus a sweep index, and nothing else.
 *   5. U = floor(x W / 2^32) from the full 64-bit product; the new height is the smallest k with C_k > U.  W = 0 (only a table with
 *      T[0] = 0 gives it) has no such k: the column takes the height N - 1.
 *      E += a(c, k_new) - a(c, k_old); n_changed counts the updates with k_new != k_old.
 *   6. best values are taken at sweep ends only: initially best_energy = the recount of the clamped input, best_sweep = 0 and
 *      best_state = the clamped input; after sweep s a STRICTLY lower E sets best_energy, best_sweep = s + 1 (relative to the call)
 *      and best_state.  energy_hist[r][0 .. n_sweeps] (optional) holds the recount, then E after each sweep.
 *   7. so: n_sweeps = 0 is a recount and a copy; state_out may be state_in (chains do not interact); D = 1 makes every update uniform,
 *      k = floor(x N / 2^32), whatever the placement; a run cut into calls with first_sweep carried over is the unbroken run.
 * best_sweep and n_changed are int64, so that mcq_resample_device's fold takes them as seg_steps_to_best / seg_n_accepted with
 * first_step = first_sweep (steps read as sweeps).
 */
#define MCQ_MAX_HEATBATH_TABLE 512
#define MCQ_HEATBATH_WEIGHT_BITS 24

typedef struct mcq_heatbath {
    int32_t N;             /* MCQ_MIN_N .. MCQ_MAX_N_BOARD */
    int32_t mode;          /* MCQ_MODE_BOARD; full_3d is MCQ_EINVAL */
    int64_t n_chains;      /* 1 .. 2^31 - 1 */
    int64_t n_sweeps;      /* >= 0 */
    int64_t first_sweep;   /* >= 0: global index of the call's sweep 0; (first_sweep + n_sweeps) N^2 < 2^63 */
    const uint32_t* seeds; /* [n_chains] */
    const uint32_t* table; /* [n_sweeps][table_len]: T_s; may be NULL when n_sweeps = 0 */
    int64_t table_len;     /* D, 1 .. MCQ_MAX_HEATBATH_TABLE */
    const uint8_t* state_in; /* [n_chains][N*N], final_state layout */
    uint8_t* state_out;    /* [n_chains][N*N]; may be state_in */
    int32_t* energy_in;    /* optional [n_chains]: E of the (clamped) input, recounted */
    int32_t* energy_out;   /* optional [n_chains]: E of the output = energy_in + the sum of the updates' differences */
    int32_t* best_energy;  /* optional [n_chains] */
    int64_t* best_sweep;   /* optional [n_chains] */
    uint8_t* best_state;   /* optional [n_chains][N*N]; neither state_in nor state_out */
    int64_t* n_changed;    /* optional [n_chains] */
    int32_t* energy_hist;  /* optional [n_chains][hist_stride] */
    int64_t hist_stride;   /* int32 entries per chain row of energy_hist, >= n_sweeps + 1 (read only when energy_hist is given) */
} mcq_heatbath;

/* the message of the last error of the calling thread from the mcq_heatbath_* calls below (they do not set mcq_last_error()) */
const char* mcq_heatbath_last_error(void);
/* Every pointer of `q` is a DEVICE pointer.  One kernel enqueued on `hip_stream`; asynchronous: nothing is copied back and nothing
 * synchronises.  MCQ_EINVAL before any launch: mode other than board, N out of range, n_chains outside 1 .. 2^31 - 1, a negative
 * n_sweeps or first_sweep, (first_sweep + n_sweeps) N^2 >= 2^63, table_len outside 1 .. 512, a NULL seeds, state_in or state_out, a NULL
 * table with n_sweeps > 0, hist_stride < n_sweeps + 1 with energy_hist given.  NOT checked, being on the device: a table with
 * T[0] = 0 can give W = 0, and the column then takes the height N - 1; nothing leaves the arrays.  An entry of T above
 * 2^MCQ_HEATBATH_WEIGHT_BITS (rule item 3) is not checked either: the sums may wrap, and the outputs are then no longer the rule's. */
int mcq_heatbath_device(const mcq_heatbath* q, void* hip_stream);
/* The same rule in plain host code over HOST buffers, same refusals; needs no GPU.  Equal to the kernel bit for bit on every output.
 * It reads the table, so it also refuses an entry above 2^MCQ_HEATBATH_WEIGHT_BITS with MCQ_EINVAL; the message names the sweep, the
 * index and the value. */
int mcq_heatbath_host(const mcq_heatbath* q);
/* The counter form of the same sweep for N <= MCQ_MAX_N_HEATBATH_COUNTERS: the same parameter block, the same refusals, the same
 * asynchrony and the same two things NOT checked (T[0] = 0, an entry above 2^MCQ_HEATBATH_WEIGHT_BITS) as mcq_heatbath_device, and MCQ_EINVAL before any launch for a larger N (mcq_heatbath_device runs every N).  Its outputs
 * equal those of mcq_heatbath_device and of mcq_heatbath_host bit for bit: the rule above is one rule, and only the way a(c, k) is
 * obtained differs.  Take the 12 line families of the cube with in-plane direction (0,1), (1,0), (1,1), (1,-1) and height step 0, +1,
 * -1 per cell, and let cnt_f(l) be the number of queens of the (clamped) board on line l of family f (at most N, a byte).  Then for a
 * column c = (i, j) of height h(c) and every k
 *     a(c, k) = sum over f of cnt_f(the line of family f through (i, j, k)) - 12 [k = h(c)]:
 * the column's own queen lies on all 12 lines through (i, j, h(c)) and on none of the 12 through another cell of its column.  The
 * kernel keeps the counters in LDS in place of the cells: 12 byte reads per height, and 12 decrements and 12 increments where a drawn
 * height differs from the old one. */
#define MCQ_MAX_N_HEATBATH_COUNTERS 16
int mcq_heatbath_counters_device(const mcq_heatbath* q, void* hip_stream);

/*
 * Quench of full_3d placements: the deterministic zero-temperature descent of Q queens in the N^3 cube to a local minimum under
 * single-queen moves (csrc/mcq_quench3d.hip) -- NOT a mode of the reference, which ships the ingredient
 * (State3DQueens.conflicts_for_queen, mcmc.py:185-226) and never calls it; never a default, like Philox, replica exchange, population
 * annealing, the board quench and the heat-bath sweep.  It recounts a placement's energy on the device independently of the sweep,
 * says whether the placement is a local minimum and which minimum lies below it, and hands back the per-queen conflict map.
 * mcq_quench above keeps refusing full_3d: a queen here has N^3 targets, and this is the different design.  The rule is integer-exact:
 *   1. a placement is Q triples (i, j, k) of bytes, the final_state / best_state layout of a full_3d run (3 Q bytes,
 *      mcq_state_bytes_for).  Every byte is clamped to N - 1 first.  If two queens then hold the same cell the placement is REPEATED:
 *      bit 0 of flags (MCQ_QUENCH3D_REPEATED) is set, energy_in is still the recount (a shared cell counts as an attacking pair, as
 *      _compute_energy counts it), state_out is the clamped input, energy_out = energy_in, n_moves = n_passes = 0, and conflicts holds
 *      a(q, pos(q)) of that placement.  The sweep never produces such a placement.
 *   2. two distinct cells attack each other iff the non-zero ones among |di|, |dj|, |dk| are all equal: the 13 line directions, the
 *      reference's seven predicates.  a(q, t) = the number of queens q' != q whose cell is t or attacks t
 *      (= conflicts_for_queen(q, t) for every cell t, occupied ones included); E = 1/2 sum_q a(q, pos(q)) (= _compute_energy);
 *      a <= min(Q - 1, 13 (N - 1)) <= 403.
 *   3. one PASS visits the queens in index order q = 0 .. Q - 1.  The candidates of q are the cells that hold no OTHER queen (its
 *      own cell is one of them); t* is the candidate with the smallest a(q, t), ties to the smallest cell index i N^2 + j N + k.
 *      q moves to t* iff a(q, t*) < a(q, pos(q)); E moves by the difference, one move is counted, and later queens of the pass see
 *      the move.
 *   4. passes repeat until one moves nothing (the placement is then a local minimum) or max_passes passes have run (0 = no limit).
 *      Every moving pass lowers E by at least 1, so a run ends within energy_in + 1 passes; n_passes counts the last, moveless pass
 *      too: a local minimum comes back with n_moves = 0, n_passes = 1.
 *   5. N = 2 .. MCQ_MAX_N_QUENCH3D (32: a cell index then fits 15 bits, as in the sweep's packed queen table) and
 *      2 <= Q <= N^3 - 1 (n_queens = 0 means N^2).  Everything else, N = 33 .. 64 included, is refused before any launch.
 * Chains do not interact, so state_out may be state_in.
 */
#define MCQ_MAX_N_QUENCH3D 32
#define MCQ_QUENCH3D_REPEATED 1 /* flags bit 0: two queens of the (clamped) input hold the same cell; nothing was moved */

typedef struct mcq_quench3d {
    int32_t N;            /* MCQ_MIN_N .. MCQ_MAX_N_QUENCH3D */
    int32_t n_queens;     /* Q: 2 .. N^3 - 1; 0 = N^2 */
    int64_t n_chains;     /* 1 .. 2^31 - 1 */
    int64_t max_passes;   /* >= 0; 0 = until a pass moves nothing */
    const uint8_t* state_in; /* [n_chains][Q][3], final_state layout of full_3d */
    uint8_t* state_out;   /* [n_chains][Q][3]; may be state_in */
    int32_t* energy_in;   /* optional [n_chains]: E of the (clamped) input, recounted */
    int32_t* energy_out;  /* optional [n_chains]: E of the output = energy_in + the sum of the moves' differences */
    int32_t* n_moves;     /* optional [n_chains] */
    int32_t* n_passes;    /* optional [n_chains] */
    uint16_t* conflicts;  /* optional [n_chains][Q]: a(q, pos(q)) of the OUTPUT placement; its sum is 2 energy_out */
    int32_t* flags;       /* optional [n_chains]: MCQ_QUENCH3D_* */
} mcq_quench3d;

/* the message of the last error of the calling thread from the two mcq_quench3d_* calls below (they do not set mcq_last_error()) */
const char* mcq_quench3d_last_error(void);
/* Every pointer of `q` is a DEVICE pointer.  One kernel enqueued on `hip_stream`; asynchronous: nothing is copied back and nothing
 * synchronises.  MCQ_EINVAL before any launch: a NULL block, N outside 2 .. 32 (33 .. 64 named as this build's limit), n_queens
 * outside 2 .. N^3 - 1 (0 = N^2), n_chains outside 1 .. 2^31 - 1, a negative max_passes, a NULL state_in or state_out. */
int mcq_quench3d_device(const mcq_quench3d* q, void* hip_stream);
/* The same rule in plain host code over HOST buffers, same refusals; needs no GPU.  Equal to the kernel bit for bit on every output;
 * exported for the tests the way mcq_quench_host is. */
int mcq_quench3d_host(const mcq_quench3d* q);

/*
 * Heat-bath queen sweeps of full_3d placements (csrc/mcq_heatbath3d.hip) -- NOT a mode of the reference, whose only move is one random
 * queen, one random cell and one Metropolis test; never a default, like Philox, replica exchange, population annealing, the two quenches
 * and the board heat-bath.  With queen q taken out, the attack field of mcq_quench3d holds a(q, t) of every cell at once, so a queen's
 * new cell is DRAWN from the Boltzmann weights of all its N^3 - Q + 1 targets and no proposal is rejected.  mcq_heatbath above keeps
 * refusing full_3d.  The rule is integer-exact:
 *   1. a placement is Q byte triples (i, j, k) in the final_state layout of full_3d (3 Q bytes); every byte is clamped to N - 1 first.
 *      N = 2 .. MCQ_MAX_N_QUENCH3D, 2 <= Q <= N^3 - 1 (n_queens = 0 means N^2).  The attack, a(q, t) and E are those of the
 *      mcq_quench3d rule above, items 1 - 2.  A REPEATED placement (two queens in one cell after clamping) sets bit 0 of flags
 *      (MCQ_HEATBATH3D_REPEATED) and no sweep is run on it: state_out = best_state = the clamped input, energy_in = energy_out =
 *      best_energy = the recount (a shared cell counts as a pair), best_sweep = n_changed = 0, and every entry of energy_hist holds the
 *      recount.
 *   2. a call runs n_sweeps sweeps; sweep s of the call has the global index g = first_sweep + s and visits the queens q = 0 .. Q - 1 in
 *      index order.  Later queens see earlier moves.  No queen is skipped: one with a = 0 is updated like any other.
 *   3. for queen q at cell p: the candidates are the cells that hold no OTHER queen (its own cell is one of them), taken in the order
 *      of the cell index t = i N^2 + j N + k.  a_min = the smallest a(q, t) over the candidates; w_t = T_s[min(a(q, t) - a_min, D - 1)]
 *      for a candidate and 0 for an occupied cell, T_s = the caller's row for sweep s (uint32, D = table_len entries,
 *      1 <= D <= MCQ_MAX_HEATBATH_TABLE; the rows of the board heat-bath, T[d] = floor(2^24 exp(-beta_s d)); a <= 403 < 512).
 *      C_t = w_0 + .. + w_t over ALL cells in index order, in uint64; W = C_{N^3 - 1} <= 2^15 2^24 = 2^39.  Every entry of T is at
 *      most 2^MCQ_HEATBATH_WEIGHT_BITS = 2^24, in a caller's own table too: the kernel adds up to 34 consecutive w_t in 32 bits before
 *      it goes to 64, and 34 * 2^24 < 2^30.
 *   4. two 32-bit words per (chain, sweep, queen): with u = g Q + q (64-bit) they are the words 2 u and 2 u + 1 of the stream
 *      word w = philox4x32-10(counter = (low 32 bits of w / 4, high bits of w / 4, 0, 0), key = (seeds[r], 2))[w % 4] -- key word 0 is
 *      MCQ_RNG_PHILOX4X32_10 of the sweep and 1 the board heat-bath, so the three streams are independent.  Both words lie in block
 *      u / 2, so one block serves two queens.  x = word 2 u | word (2 u + 1) << 32.
 *   5. U = floor(x W / 2^64), the high half of the 64 x 64 product; the new cell is the smallest t with C_t > U.  W = 0 (only a table
 *      with T[0] = 0 gives it, which cannot be checked on the device) leaves the queen where it is.  E += a(q, t_new) - a(q, p);
 *      n_changed counts the updates with t_new != p.
 *   6. best values are taken at sweep ends only: initially best_energy = the recount of the clamped input, best_sweep = 0 and
 *      best_state = the clamped input; after sweep s a STRICTLY lower E sets best_energy, best_sweep = s + 1 (relative to the call)
 *      and best_state.  energy_hist[r][0 .. n_sweeps] (optional) holds the recount, then E after each sweep.  n_sweeps = 0 is a
 *      recount and a copy.  The state of a chain is its placement plus a sweep index, and nothing else: a run cut into calls with
 *      first_sweep carried over is the unbroken run.  state_out may be state_in (chains do not interact).
 *   7. D = 1 makes every update uniform over the candidates, whatever the placement: the new cell is the floor(x F / 2^64)-th
 *      candidate in index order, F = N^3 - Q + 1.
 * best_sweep and n_changed are int64, so that mcq_resample_device's fold takes them as seg_steps_to_best / seg_n_accepted with
 * first_step = first_sweep (steps read as sweeps), as with mcq_heatbath.
 */
#define MCQ_HEATBATH3D_REPEATED 1 /* flags bit 0: two queens of the (clamped) input hold the same cell; no sweep was run */

typedef struct mcq_heatbath3d {
    int32_t N;             /* MCQ_MIN_N .. MCQ_MAX_N_QUENCH3D */
    int32_t n_queens;      /* Q: 2 .. N^3 - 1; 0 = N^2 */
    int64_t n_chains;      /* 1 .. 2^31 - 1 */
    int64_t n_sweeps;      /* >= 0 */
    int64_t first_sweep;   /* >= 0: global index of the call's sweep 0; (first_sweep + n_sweeps) Q < 2^62 */
    const uint32_t* seeds; /* [n_chains] */
    const uint32_t* table; /* [n_sweeps][table_len]: T_s; may be NULL when n_sweeps = 0 */
    int64_t table_len;     /* D, 1 .. MCQ_MAX_HEATBATH_TABLE */
    const uint8_t* state_in; /* [n_chains][Q][3], final_state layout of full_3d */
    uint8_t* state_out;    /* [n_chains][Q][3]; may be state_in */
    int32_t* energy_in;    /* optional [n_chains]: E of the (clamped) input, recounted */
    int32_t* energy_out;   /* optional [n_chains]: E of the output = energy_in + the sum of the updates' differences */
    int32_t* best_energy;  /* optional [n_chains] */
    int64_t* best_sweep;   /* optional [n_chains] */
    uint8_t* best_state;   /* optional [n_chains][Q][3]; neither state_in nor state_out */
    int64_t* n_changed;    /* optional [n_chains] */
    int32_t* energy_hist;  /* optional [n_chains][hist_stride] */
    int64_t hist_stride;   /* int32 entries per chain row of energy_hist, >= n_sweeps + 1 (read only when energy_hist is given) */
    int32_t* flags;        /* optional [n_chains]: MCQ_HEATBATH3D_* */
} mcq_heatbath3d;

/* the message of the last error of the calling thread from the two mcq_heatbath3d_* calls below (they do not set mcq_last_error()) */
const char* mcq_heatbath3d_last_error(void);
/* Every pointer of `q` is a DEVICE pointer.  One kernel enqueued on `hip_stream`; asynchronous: nothing is copied back and nothing
 * synchronises.  MCQ_EINVAL before any launch: a NULL block, seeds, state_in or state_out, a NULL table with n_sweeps > 0, N outside
 * 2 .. 32 (33 .. 64 named as this build's limit), n_queens outside 2 .. N^3 - 1 (0 = N^2), n_chains outside 1 .. 2^31 - 1, a negative
 * n_sweeps or first_sweep, (first_sweep + n_sweeps) Q >= 2^62, table_len outside 1 .. 512, hist_stride < n_sweeps + 1 with
 * energy_hist given.  NOT checked, being on the device: a table with T[0] = 0 can give W = 0, and the queen then stays where it is; an
 * entry of T above 2^MCQ_HEATBATH_WEIGHT_BITS (rule item 3) can wrap a 32-bit partial sum, and the outputs are then no longer the rule's. */
int mcq_heatbath3d_device(const mcq_heatbath3d* q, void* hip_stream);
/* The same rule in plain host code over HOST buffers, same refusals; needs no GPU.  Equal to the kernel bit for bit on every output.
 * It reads the table, so it also refuses an entry above 2^MCQ_HEATBATH_WEIGHT_BITS with MCQ_EINVAL; the message names the sweep, the
 * index and the value. */
int mcq_heatbath3d_host(const mcq_heatbath3d* q);

/*
 * Parallel tempering of board heat-bath sweeps, one ladder per workgroup (csrc/mcq_temper.hip) -- NOT a mode of the reference, never a
 * default, like Philox, replica exchange in the Metropolis sweep (mcq_params.exchange_*), population annealing, the quenches and the
 * heat baths.  The replicas of a ladder run mcq_heatbath's sweep at different beta and trade their temperatures between sweeps, in ONE
 * launch: mcq_heatbath takes one table row per sweep for every chain of a launch, and chains of different workgroups cannot meet
 * without ending the kernel.  Boards only (full_3d placements: mcq_temper3d below).  The rule is integer-exact, with no floating point on the device:
 *   1. ladders: R = replicas is 2, 4, 8 or 16 and divides n_chains; ladder g holds the chain slots [g R, (g + 1) R).  A slot keeps its
 *      placement, its seed, its Philox stream, its best values and its history for the whole run; what moves between the slots of a
 *      ladder is the RUNG t = 0 .. R - 1.  rung_in (optional) gives every slot's starting rung and must hold a permutation of 0 .. R - 1
 *      per ladder; NULL means slot r starts on rung r mod R.  rung_out (optional) returns the final rungs.
 *   2. the sweep: a call runs n_sweeps sweeps; sweep s of the call has the global index g = first_sweep + s and is the sweep of the
 *      mcq_heatbath rule above, items 1 - 6, unchanged except for the table row: a slot on rung t uses the row T[s][t] of `table`
 *      (uint32 [n_sweeps][R][table_len]).  Unchanged means the same clamping, the same a(c, k), the same column order, the same word
 *      w = g N^2 + c of the Philox stream with key (seeds[slot], 1), the same U and selection, the same best values at sweep ends
 *      (before the sweep's event) and the same energy_hist.  A ladder whose R rows are equal is therefore R plain heat-bath chains,
 *      whatever the exchanges do.  mcq_temper_counters_device below is a second way to obtain a(c, k), not a second rule.
 *   3. the exchange: exchange_every = K >= 1.  After the sweep with global index g an EVENT happens when (g + 1) mod K = 0; its global
 *      index is e = (g + 1) / K - 1.  The event looks at the pairs of neighbouring rungs (t, t + 1) with t = e (mod 2) and t + 1 < R.
 *      With a the slot on rung t, b the slot on rung t + 1 and Delta = E_b - E_a, the running energies after that sweep:
 *        Delta >= 0  the colder rung holds the higher energy (or the same): the two slots swap rungs;
 *        Delta <  0  d = -Delta, and they swap when x < X[j][t][min(d, DX - 1)],
 *      where `swap_table` is uint32 [n_events][R - 1][swap_len], j = e - floor(first_sweep / K) is the event's index within the call,
 *      DX = swap_len (1 .. MCQ_MAX_TEMPER_SWAP_TABLE), and x is the word e R + t (64-bit) of the stream
 *      word w = philox4x32-10(counter = (low 32 bits of w / 4, high bits of w / 4, 0, 0), key = (seeds[g R], 3))[w % 4] -- the seed of
 *      the ladder's slot 0; key words 0, 1 and 2 are taken by MCQ_RNG_PHILOX4X32_10 of the sweep and the two heat baths.  The pairs of
 *      an event are disjoint, so their order does not matter.  x is drawn only where Delta < 0 (a stream addressed by position).
 *      n_events = floor((first_sweep + n_sweeps) / K) - floor(first_sweep / K), and the caller must say as many;
 *      floor((first_sweep + n_sweeps) / K) R must stay below 2^63.
 *   4. the Python side builds T[s][t][d] = floor(2^24 exp(-beta_s l_t d)) (the rows of mcq_heatbath at beta_s l_t) and
 *      X[j][t][d] = min(2^32 - 1, floor(2^32 exp(-beta_g (l_{t+1} - l_t) d))), g the sweep the event follows, from multipliers
 *      0 < l_0 <= l_1 <= .. <= l_{R-1}: rung R - 1 is the coldest, and the swap probability min(1, exp((beta_b - beta_a)(E_b - E_a)))
 *      of replica exchange is 1 for Delta >= 0, which is why the table is one-sided.  A caller's own tables are as good; every entry
 *      of T is at most 2^MCQ_HEATBATH_WEIGHT_BITS.
 *   5. outputs per slot: those of mcq_heatbath (relative to the call, as there), rung_out, n_exchanges (the swaps of this call the slot
 *      took part in) and rung_hist (optional, uint8 [n_chains][hist_stride]: entry 0 the starting rung, entry s + 1 the rung after
 *      sweep s and its event).  Per ladder: pair_accepted (optional, int64 [n_chains / R][R - 1]: the swaps of this call per pair of
 *      rungs (t, t + 1)), which a caller needs to tune a ladder.  The sum of n_exchanges over a ladder is twice that of pair_accepted.
 *   6. so: the state of a ladder is its placements, its rungs and a sweep index, and nothing else: a run cut into calls with
 *      first_sweep, the placements and the rungs carried over (and the rows of both tables split accordingly) is the unbroken run.
 *      K > n_sweeps + first_sweep gives no event: each slot is then a plain heat-bath chain at its own rung's rows.  state_out may be
 *      state_in (the slots of a ladder meet through their energies only).
 */
#define MCQ_MAX_TEMPER_SWAP_TABLE 4096
#define MCQ_MAX_TEMPER_LDS (160 * 1024) /* bytes of LDS a workgroup of mcq_temper_device may take */

typedef struct mcq_temper {
    int32_t N;             /* MCQ_MIN_N .. MCQ_MAX_N_BOARD (mcq_temper_device: as far as a ladder fits the LDS, see below) */
    int32_t mode;          /* MCQ_MODE_BOARD; full_3d is MCQ_EINVAL */
    int64_t n_chains;      /* 1 .. 2^31 - 1, a multiple of replicas */
    int64_t n_sweeps;      /* >= 0 */
    int64_t first_sweep;   /* >= 0: global index of the call's sweep 0; (first_sweep + n_sweeps) N^2 < 2^63 */
    int64_t replicas;      /* R: 2, 4, 8 or 16 */
    int64_t exchange_every; /* K >= 1 */
    int64_t n_events;      /* floor((first_sweep + n_sweeps) / K) - floor(first_sweep / K): the rows of swap_table */
    const uint32_t* seeds; /* [n_chains] */
    const uint32_t* table; /* [n_sweeps][R][table_len]: T; may be NULL when n_sweeps = 0 */
    int64_t table_len;     /* D, 1 .. MCQ_MAX_HEATBATH_TABLE */
    const uint32_t* swap_table; /* [n_events][R - 1][swap_len]: X; may be NULL when n_events = 0 */
    int64_t swap_len;      /* DX, 1 .. MCQ_MAX_TEMPER_SWAP_TABLE */
    const uint8_t* rung_in; /* optional [n_chains]: a permutation of 0 .. R - 1 per ladder; NULL = slot r on rung r mod R */
    uint8_t* rung_out;     /* optional [n_chains] */
    const uint8_t* state_in; /* [n_chains][N*N], final_state layout */
    uint8_t* state_out;    /* [n_chains][N*N]; may be state_in */
    int32_t* energy_in;    /* optional [n_chains]: E of the (clamped) input, recounted */
    int32_t* energy_out;   /* optional [n_chains] */
    int32_t* best_energy;  /* optional [n_chains] */
    int64_t* best_sweep;   /* optional [n_chains] */
    uint8_t* best_state;   /* optional [n_chains][N*N]; neither state_in nor state_out */
    int64_t* n_changed;    /* optional [n_chains] */
    int32_t* energy_hist;  /* optional [n_chains][hist_stride] */
    int64_t hist_stride;   /* entries per chain row of energy_hist and of rung_hist, >= n_sweeps + 1 (read only when one of them is given) */
    int64_t* n_exchanges;  /* optional [n_chains] */
    uint8_t* rung_hist;    /* optional [n_chains][hist_stride] */
    int64_t* pair_accepted; /* optional [n_chains / R][R - 1] */
} mcq_temper;

/* the message of the last error of the calling thread from the two mcq_temper_* calls below (they do not set mcq_last_error()) */
const char* mcq_temper_last_error(void);
/* Every pointer of `q` is a DEVICE pointer.  ONE kernel enqueued on `hip_stream`, a workgroup per ladder (two ladders where one is
 * narrower than a wavefront), the exchange through LDS and two barriers; asynchronous: nothing is copied back and nothing synchronises.
 * MCQ_EINVAL before any launch and without touching a device: what mcq_heatbath_device refuses of the fields the two blocks share;
 * replicas other than 2, 4, 8, 16 or not dividing n_chains; exchange_every < 1; an n_events other than rule item 3 gives;
 * floor((first_sweep + n_sweeps) / K) R >= 2^63; swap_len outside 1 .. MCQ_MAX_TEMPER_SWAP_TABLE; a NULL swap_table with n_events > 0;
 * hist_stride < n_sweeps + 1 with energy_hist or rung_hist given; and a ladder whose LDS -- per ladder 6 NP^2 R bytes of placements (NP = N rounded up to
 * 8, 12, 16, 24, 32 or 64), 4 R table_len bytes of staged rows and 12 R bytes for the event -- exceeds MCQ_MAX_TEMPER_LDS: N = 33 .. 64 with R >= 8, and every
 * N > 64; the message names N, R and the bytes.  NOT checked, being on the device: what mcq_heatbath_device does not check of T, and
 * rung_in -- a rung is clamped to R - 1, and a ladder whose rungs are no permutation gets outputs that are not the rule's; nothing
 * leaves the arrays. */
int mcq_temper_device(const mcq_temper* q, void* hip_stream);
/* The counter form of the same tempered sweep for N <= MCQ_MAX_N_TEMPER_COUNTERS: the same parameter block, the same asynchrony, the
 * same refusals before any launch (through mcq_temper_last_error) and the same things NOT checked as mcq_temper_device, and MCQ_EINVAL
 * before any launch for a larger N; the message names 16.  This is a second way to obtain a(c, k) -- the per-line queen counters of
 * mcq_heatbath_counters_device above, one region per slot in the LDS of the ladder's workgroup -- and there is one rule: the outputs
 * equal those of mcq_temper_device and of mcq_temper_host bit for bit.  A slot's counters stay with the slot at an exchange; only the
 * rung moves.  LDS per ladder: R regions of 1 856, 4 288 or 7 616 bytes (N up to 8, 12, 16), 4 R table_len bytes of staged rows and
 * 12 R bytes for the event, two ladders per workgroup at R = 2: at most 154 816 bytes (N = 16, R = 16, table_len = 512), so every
 * block with N <= 16 that passes the checks fits MCQ_MAX_TEMPER_LDS. */
#define MCQ_MAX_N_TEMPER_COUNTERS 16
int mcq_temper_counters_device(const mcq_temper* q, void* hip_stream);
/* The same rule in plain host code over HOST buffers, for every N up to MCQ_MAX_N_BOARD (no LDS here); needs no GPU.  Equal to the
 * kernel bit for bit on every output.  It reads its inputs, so it also refuses with MCQ_EINVAL an entry of T above
 * 2^MCQ_HEATBATH_WEIGHT_BITS and a rung_in that is no permutation of 0 .. R - 1 in some ladder; the message names the place. */
int mcq_temper_host(const mcq_temper* q);

/*
 * Parallel tempering of full_3d heat-bath queen sweeps, one ladder per workgroup (csrc/mcq_temper3d.hip) -- NOT a mode of the reference,
 * never a default, like everything above that is labelled so.  The replicas of a ladder run mcq_heatbath3d's sweep at different beta, each
 * on an attack field of its own, and trade their temperatures between sweeps, in ONE launch.  mcq_temper above keeps refusing full_3d;
 * this block has its own entry points.  The rule is integer-exact, with no floating point on the device:
 *   1. ladders: as in the mcq_temper rule, item 1.  R = replicas is 2, 4, 8 or 16 and divides n_chains; ladder g holds the chain slots
 *      [g R, (g + 1) R).  A slot keeps its placement, its seed, its stream, its best values and its histories; what moves is the RUNG.
 *      rung_in and rung_out are as there.
 *   2. the sweep is that of the mcq_heatbath3d rule, items 1 - 7, unchanged except for the table row: a slot on rung t uses the row
 *      T[s][t] of `table` (uint32 [n_sweeps][R][table_len]).  Unchanged means the same clamping, the same cell order, the same update
 *      word u = g Q + q of the stream with key (seeds[slot], 2), the same U and selection, the same W = 0 case, and the same best values
 *      at sweep ends (taken before the sweep's event).  A ladder whose R rows are equal is therefore R plain mcq_heatbath3d chains,
 *      whatever the exchanges do.
 *   3. the exchange is that of the mcq_temper rule, item 3, verbatim -- the event after the sweep with global index g when
 *      (g + 1) mod K = 0, the pairs t = e (mod 2), Delta >= 0 always swaps and otherwise x < X[j][t][min(-Delta, DX - 1)], x the word
 *      e R + t -- with one change: the key of the stream is (seeds[g R], 4); key words 0 - 3 are taken by the sweep, the two heat baths
 *      and mcq_temper.  The bounds on n_events, swap_len and the word index are the same.
 *   4. a REPEATED placement (two queens in one cell after clamping) cannot enter a byte field.  If any slot of a ladder holds one, the
 *      whole ladder is HELD, handed back unmoved: every slot gets state_out = best_state = the clamped input, energy_in = energy_out =
 *      best_energy = the pairwise recount (a shared cell counts as a pair), best_sweep = n_changed = n_exchanges = 0, rung_out = its
 *      starting rung, every entry of energy_hist the recount and every entry of rung_hist the starting rung; the ladder's row of
 *      pair_accepted is 0.  flags bit 0 (MCQ_HEATBATH3D_REPEATED) is set on the slots that hold a repeat, bit 1 (MCQ_TEMPER3D_HELD) on
 *      every slot of such a ladder.  The host code and the kernel do the same (it keeps every barrier of the kernel uniform over the
 *      workgroup).  Other ladders of the call run normally.
 *   5. outputs, segments and K > number of sweeps: as in the mcq_temper rule, items 5 - 6.  The state of a ladder is its placements, its
 *      rungs and a sweep index: a run cut into calls with those carried over, and the rows of both tables split accordingly, is the
 *      unbroken run.  state_out may be state_in.
 * The tables are those of mcq_temper, item 4: T[s][t][d] = floor(2^24 exp(-beta_s l_t d)), a <= 403 < 512.
 *
 * mcq_temper3d_device keeps a ladder in the LDS of one workgroup: per chain 72 dwords of its own (minimum, scan, winner), the field
 * (one byte per cell to N = 19, 16 bits beyond), the occupancy bitmap and the queens (16 bits each), rounded up to 4 dwords; R D dwords
 * of staged table rows; 3 R words for the event:
 *   bytes = 4 (R roundup4(72 + fw + bw + ceil(Q / 2)) + R D + 3 R) <= MCQ_MAX_TEMPER_LDS - MCQ_TEMPER3D_STATIC_LDS,
 *   fw = ceil(N^3 / (4 or 2)),  bw = ceil(N^3 / 32); the workgroup-wide OR behind "some slot repeats" keeps 256 bytes of static LDS.
 * With Q = N^2 and D = 512 (a shorter table lets a slightly larger N in) the largest N of each R, and its bytes:
 *      R = 16   N = 18   153 024          R = 4   N = 25   147 248
 *      R = 8    N = 20   161 248          R = 2   N = 32   148 056
 * (N = 12, R = 16 with Q = N^3 - 1 = 1727: 124 096.)  A chain is W = min(64 | 256 | 1024 for N <= 12 | <= 19 | <= 32, 1024 / R) lanes; a
 * lane adds the weights of (ceil(fw / W) | 1) cells-per-dword cells in 32 bits, at most 108 cells in what fits the LDS (N = 19, R = 16,
 * which fits with a table shorter than 512), and 255 entries of 2^24 stay below 2^32.
 */
#define MCQ_TEMPER3D_STATIC_LDS 256 /* bytes of static LDS of the kernel, which count against MCQ_MAX_TEMPER_LDS */
#define MCQ_TEMPER3D_HELD 2 /* flags bit 1: a slot of this ladder holds a repeated placement; the whole ladder was handed back unmoved */

typedef struct mcq_temper3d {
    int32_t N;             /* MCQ_MIN_N .. MCQ_MAX_N_QUENCH3D (mcq_temper3d_device: as far as a ladder fits the LDS, see above) */
    int32_t n_queens;      /* Q: 2 .. N^3 - 1; 0 = N^2 */
    int64_t n_chains;      /* 1 .. 2^31 - 1, a multiple of replicas */
    int64_t n_sweeps;      /* >= 0 */
    int64_t first_sweep;   /* >= 0: global index of the call's sweep 0; (first_sweep + n_sweeps) Q < 2^62 */
    int64_t replicas;      /* R: 2, 4, 8 or 16 */
    int64_t exchange_every; /* K >= 1 */
    int64_t n_events;      /* floor((first_sweep + n_sweeps) / K) - floor(first_sweep / K): the rows of swap_table */
    const uint32_t* seeds; /* [n_chains] */
    const uint32_t* table; /* [n_sweeps][R][table_len]: T; may be NULL when n_sweeps = 0 */
    int64_t table_len;     /* D, 1 .. MCQ_MAX_HEATBATH_TABLE */
    const uint32_t* swap_table; /* [n_events][R - 1][swap_len]: X; may be NULL when n_events = 0 */
    int64_t swap_len;      /* DX, 1 .. MCQ_MAX_TEMPER_SWAP_TABLE */
    const uint8_t* rung_in; /* optional [n_chains]: a permutation of 0 .. R - 1 per ladder; NULL = slot r on rung r mod R */
    uint8_t* rung_out;     /* optional [n_chains] */
    const uint8_t* state_in; /* [n_chains][Q][3], final_state layout of full_3d */
    uint8_t* state_out;    /* [n_chains][Q][3]; may be state_in */
    int32_t* energy_in;    /* optional [n_chains]: E of the (clamped) input, recounted */
    int32_t* energy_out;   /* optional [n_chains] */
    int32_t* best_energy;  /* optional [n_chains] */
    int64_t* best_sweep;   /* optional [n_chains] */
    uint8_t* best_state;   /* optional [n_chains][Q][3]; neither state_in nor state_out */
    int64_t* n_changed;    /* optional [n_chains] */
    int32_t* energy_hist;  /* optional [n_chains][hist_stride] */
    int64_t hist_stride;   /* entries per chain row of energy_hist and of rung_hist, >= n_sweeps + 1 (read only when one of them is given) */
    int64_t* n_exchanges;  /* optional [n_chains] */
    uint8_t* rung_hist;    /* optional [n_chains][hist_stride] */
    int64_t* pair_accepted; /* optional [n_chains / R][R - 1] */
    int32_t* flags;        /* optional [n_chains]: MCQ_HEATBATH3D_REPEATED | MCQ_TEMPER3D_HELD */
} mcq_temper3d;

/* the message of the last error of the calling thread from the two mcq_temper3d_* calls below (they do not set mcq_last_error()) */
const char* mcq_temper3d_last_error(void);
/* Every pointer of `q` is a DEVICE pointer.  ONE kernel enqueued on `hip_stream`, a workgroup per ladder, the exchange through LDS and
 * two barriers; asynchronous: nothing is copied back and nothing synchronises.  MCQ_EINVAL before any launch and without touching a
 * device: what mcq_heatbath3d_device and mcq_temper_device refuse of the fields they share with this block, and any (N, R, Q, table_len)
 * whose ladder exceeds MCQ_MAX_TEMPER_LDS (the message names N, R, Q and the bytes) or whose lanes would add more than 255 weights in
 * 32 bits.  NOT checked, being on the device: what mcq_heatbath3d_device does not check of T, and rung_in -- a rung is clamped to
 * R - 1, and a ladder whose rungs are no permutation gets outputs that are not the rule's; nothing leaves the arrays. */
int mcq_temper3d_device(const mcq_temper3d* q, void* hip_stream);
/* The same rule in plain host code over HOST buffers, for every N up to MCQ_MAX_N_QUENCH3D and every R (no LDS here); needs no GPU.
 * Equal to the kernel bit for bit on every output.  It reads its inputs, so it also refuses with MCQ_EINVAL an entry of T above
 * 2^MCQ_HEATBATH_WEIGHT_BITS and a rung_in that is no permutation of 0 .. R - 1 in some ladder; the message names the place. */
int mcq_temper3d_host(const mcq_temper3d* q);

/*
 * Pair-move quench: the deterministic descent of board placements to a minimum under single-height moves AND under moves of two
 * columns at once (csrc/mcq_quench_pairs.hip) -- NOT a mode of the reference; never a default, like Philox, replica exchange,
 * population annealing, the quenches, the heat baths and the tempered sweeps.  mcq_quench above certifies a placement against the
 * single-move neighbourhood; this block tests it against the smallest larger one and descends below it.  Boards only.  The rule is
 * integer-exact:
 *   1. every input byte is clamped to N - 1 first; a(c, k) and E are those of the mcq_quench rule, items 1 - 2.  Two columns
 *      c = (i, j) != c' = (i', j') are ALIGNED when di = 0 or dj = 0 or |di| = |dj| (they share a row, a column or a diagonal of the
 *      board).  att((c, k), (c', k')) = 1 when the columns are aligned and |k - k'| = 0 or d, d = max(|di|, |dj|); otherwise 0.
 *   2. DESCENT: passes of the mcq_quench rule, items 3 - 4, until a pass moves nothing; there is no pass limit.  n_moves counts the
 *      single moves of all descents of the run.  energy_single is E after the FIRST descent: what mcq_quench returns with
 *      max_passes = 0.
 *   3. SCAN: the candidates are (c1, c2, k1, k2) with c1 < c2 (row-major indices), the two columns aligned, k1 != h(c1) and
 *      k2 != h(c2).  With h1 = h(c1), h2 = h(c2):
 *        D = a(c1, k1) - a(c1, h1) + a(c2, k2) - a(c2, h2)
 *            - att((c1, k1), (c2, h2)) - att((c1, h1), (c2, k2)) + att((c1, h1), (c2, h2)) + att((c1, k1), (c2, k2))
 *      which is the change of E when both heights change at once.  The scan takes the candidate with the lexicographically smallest
 *      (D, c1, c2, k1, k2).  n_rounds counts the scans.
 *   4. if that D >= 0 the run ends with certified = 1: no single move and no pair move lowers E.  (A pair of columns that are not
 *      aligned has D = the sum of two single-move differences, which are >= 0 behind a descent: it cannot improve, which is why the
 *      candidates are the aligned pairs.)  Otherwise both heights are applied, E += D, n_pair_moves grows by 1, and the run goes back
 *      to item 2.  When max_rounds > 0 and n_rounds has reached it after an applied move, one more descent runs and the run ends
 *      with certified = 0.  Every pair move lowers E by at least 1, so a run ends within energy_in + 1 rounds; a 2-move minimum comes
 *      back with n_pair_moves = 0, n_rounds = 1, certified = 1.
 * An implementation may skip candidates that cannot have D < 0 -- behind a descent both single-move differences are >= 0 and the four
 * att terms add at least -2, so D < 0 needs them to sum to at most 1 --; it may not change the result.
 * N = MCQ_MIN_N .. MCQ_MAX_N_QUENCH_PAIRS on the device and in host code alike: every a(c, k) is at most 4 (N - 1) = 124 there and
 * fits a byte.  Chains do not interact, so state_out may be state_in.
 */
#define MCQ_MAX_N_QUENCH_PAIRS 32
typedef struct mcq_quench_pairs {
    int32_t N;              /* MCQ_MIN_N .. MCQ_MAX_N_QUENCH_PAIRS */
    int32_t mode;           /* MCQ_MODE_BOARD; anything else is MCQ_EINVAL */
    int64_t n_chains;       /* 1 .. 2^31 - 1 */
    int64_t max_rounds;     /* >= 0; 0 = until a scan finds no improving pair */
    const uint8_t* state_in; /* [n_chains][N*N], final_state layout */
    uint8_t* state_out;     /* [n_chains][N*N]; may be state_in */
    int32_t* energy_in;     /* optional [n_chains]: E of the (clamped) input, recounted */
    int32_t* energy_single; /* optional [n_chains]: E after the first descent */
    int32_t* energy_out;    /* optional [n_chains]: E of the output */
    int32_t* n_moves;       /* optional [n_chains]: single moves of all descents */
    int32_t* n_pair_moves;  /* optional [n_chains] */
    int32_t* n_rounds;      /* optional [n_chains]: scans */
    int32_t* certified;     /* optional [n_chains]: 1 = the last scan found no improving pair, 0 = max_rounds ended the run */
    uint16_t* conflicts;    /* optional [n_chains][N*N]: a(c, h(c)) of the OUTPUT placement; its sum is 2 energy_out */
} mcq_quench_pairs;

/* the message of the last error of the calling thread from the two mcq_quench_pairs_* calls below (they do not set mcq_last_error()) */
const char* mcq_quench_pairs_last_error(void);
/* Every pointer of `q` is a DEVICE pointer.  One kernel enqueued on `hip_stream`; asynchronous: nothing is copied back and nothing
 * synchronises.  MCQ_EINVAL before any launch: mode other than board, N out of range, n_chains outside 1 .. 2^31 - 1, a negative
 * max_rounds, a NULL state_in or state_out. */
int mcq_quench_pairs_device(const mcq_quench_pairs* q, void* hip_stream);
/* The same rule in plain host code over HOST buffers, same refusals; needs no GPU.  Equal to the kernel bit for bit on every output. */
int mcq_quench_pairs_host(const mcq_quench_pairs* q);

/*
 * Basin hopping (iterated local search) of board placements: kick a few columns of a minimum, descend again, keep the new minimum
 * when it is no worse and go back otherwise (csrc/mcq_hop.hip) -- NOT a mode of the reference; never a default, like Philox, replica
 * exchange, population annealing, the quenches, the heat baths and the tempered sweeps.  The thermal searches end on minima that
 * mcq_quench and mcq_quench_pairs certify; this block goes on from a minimum.  Boards only.  The rule is integer-exact:
 *   1. every input byte is clamped to N - 1 first; a(c, k), E, "aligned" and att are those of the mcq_quench rule, items 1 - 2, and
 *      of the mcq_quench_pairs rule, item 1.
 *   2. LOCAL SEARCH L, by local_search:
 *        MCQ_HOP_SINGLE  the DESCENT of mcq_quench_pairs, item 2: passes of the mcq_quench rule until one moves nothing
 *                        (mcq_quench with max_passes = 0);
 *        MCQ_HOP_PAIRS   the whole mcq_quench_pairs run with max_rounds = 0: descent, scan, apply and descent again, until a scan
 *                        finds no improving pair.
 *      A placement that L returns is a fixed point of L: L moves nothing on it.
 *   3. a call first applies L to the clamped input: energy_in is the recount before it, energy_start is E behind it.  Then it runs
 *      n_hops hops; hop t = 0 .. n_hops - 1 of the call has the GLOBAL index g = first_hop + t.
 *   4. KICK of hop g, with m = kick (1 .. MCQ_MAX_HOP_KICK): for q = 0 .. m - 1 in order, with x1 = word 2 (g m + q) and
 *      x2 = word 2 (g m + q) + 1 of the chain's stream,  c = floor(x1 N^2 / 2^32),  k = floor(x2 N / 2^32),  and h(c) = k.  Later
 *      kicks of the hop see earlier ones; a column may be drawn twice; k may equal h(c).  Word w (64-bit) of chain r is
 *        philox4x32-10(counter = (low 32 bits of w / 4, high bits of w / 4, 0, 0), key = (seeds[r], 5))[w % 4]
 *      (key words 0 - 4 are taken by the sweep, the two heat baths and the two tempered sweeps).
 *   5. L runs on the kicked placement and gives E'.  The hop is ACCEPTED when E' <= E + slack, E the energy BEFORE the kick: the
 *      placement and E' stay.  Otherwise every height returns to what it was before the kick, and so does E.  n_accepted counts the
 *      accepted hops, those that land on the placement they left too.
 *   6. best_energy = energy_start, best_hop = 0 and best_state = the placement behind item 3 to begin with.  An accepted hop with E'
 *      strictly below best_energy sets best_energy, best_hop = t + 1 (relative to the call) and best_state, and counts in n_improved.
 *      energy_hist[r][0 .. n_hops] holds energy_start, then E after each hop.
 *   7. n_moves and n_pair_moves count the single and pair moves of every L of the call: that of item 3 and those of rejected hops
 *      too.
 * Consequences: n_hops = 0 is L alone -- mcq_quench_pairs with max_rounds = 0 (MCQ_HOP_PAIRS) or mcq_quench with max_passes = 0
 * (MCQ_HOP_SINGLE).  The state of a chain is its placement plus a hop index and nothing else: a run cut into calls, each fed the
 * state_out of the one before and first_hop carried over, is the unbroken run, because item 3 moves nothing on a fixed point of L.
 * (Of the cut run's figures n_accepted, n_moves and n_pair_moves add up, energy_out and state are the last call's, and best_* are
 * those of the FIRST call with the smallest best_energy, its best_hop moved by the hops before that call.  n_improved does not add
 * up when slack > 0: a call counts against its own energy_start, which may lie above an earlier call's best_energy; the whole run's
 * count is the number of new lows of the joined energy_hist.)  Chains do not interact, so state_out may be
 * state_in.  N = MCQ_MIN_N .. MCQ_MAX_N_QUENCH_PAIRS on the device and in host code alike.
 */
#define MCQ_HOP_SINGLE 0
#define MCQ_HOP_PAIRS 1
#define MCQ_MAX_HOP_KICK 1024
typedef struct mcq_hop {
    int32_t N;              /* MCQ_MIN_N .. MCQ_MAX_N_QUENCH_PAIRS */
    int32_t mode;           /* MCQ_MODE_BOARD; anything else is MCQ_EINVAL */
    int64_t n_chains;       /* 1 .. 2^31 - 1 */
    int64_t n_hops;         /* >= 0; 0 = L alone */
    int64_t first_hop;      /* >= 0: the global index of the call's first hop; 2 kick (first_hop + n_hops) < 2^63 */
    int32_t kick;           /* 1 .. MCQ_MAX_HOP_KICK: the draws of one kick */
    int32_t slack;          /* >= 0: a hop may raise E by this much */
    int32_t local_search;   /* MCQ_HOP_SINGLE or MCQ_HOP_PAIRS */
    const uint32_t* seeds;  /* [n_chains] */
    const uint8_t* state_in; /* [n_chains][N*N], final_state layout */
    uint8_t* state_out;     /* [n_chains][N*N]; may be state_in */
    int32_t* energy_in;     /* optional [n_chains]: E of the (clamped) input, recounted */
    int32_t* energy_start;  /* optional [n_chains]: E behind the first L */
    int32_t* energy_out;    /* optional [n_chains]: E of the output */
    int32_t* best_energy;   /* optional [n_chains] */
    int64_t* best_hop;      /* optional [n_chains]: 0 = the placement behind the first L, t + 1 = behind hop t of the call */
    uint8_t* best_state;    /* optional [n_chains][N*N]; neither state_in nor state_out */
    int64_t* n_accepted;    /* optional [n_chains] */
    int64_t* n_improved;    /* optional [n_chains] */
    int64_t* n_moves;       /* optional [n_chains]: single moves of every L */
    int64_t* n_pair_moves;  /* optional [n_chains]: pair moves of every L (0 under MCQ_HOP_SINGLE) */
    int32_t* energy_hist;   /* optional [n_chains][hist_stride]: entries 0 .. n_hops */
    int64_t hist_stride;    /* >= n_hops + 1 when energy_hist is given; not read otherwise */
} mcq_hop;

/* the message of the last error of the calling thread from the two mcq_hop_* calls below (they do not set mcq_last_error()) */
const char* mcq_hop_last_error(void);
/* Every pointer of `q` is a DEVICE pointer.  One kernel enqueued on `hip_stream`, whatever n_hops is; asynchronous: nothing is
 * copied back and nothing synchronises.  MCQ_EINVAL before any launch: mode other than board, N out of range, n_chains outside
 * 1 .. 2^31 - 1, a negative n_hops, first_hop or slack, kick outside 1 .. MCQ_MAX_HOP_KICK, 2 kick (first_hop + n_hops) >= 2^63, a
 * local_search that is neither value, a NULL seeds, state_in or state_out, hist_stride below n_hops + 1 when energy_hist is given. */
int mcq_hop_device(const mcq_hop* q, void* hip_stream);
/* The same rule in plain host code over HOST buffers, same refusals; needs no GPU.  Equal to the kernel bit for bit on every output. */
int mcq_hop_host(const mcq_hop* q);

/*
 * Basin hopping (iterated local search) of full_3d placements: kick a few queens of a minimum to free cells, descend again, keep the
 * new minimum when it is no worse and go back otherwise (csrc/mcq_hop3d.hip) -- NOT a mode of the reference; never a default, like
 * everything above that is labelled so.  mcq_hop above keeps refusing full_3d: a queen here has N^3 targets, and this block has its own
 * entry points.  The rule is integer-exact:
 *   1. the placement (Q triples of bytes, 3 Q bytes per chain), the clamping to N - 1, REPEATED, a(q, t) and E are those of the
 *      mcq_quench3d rule, items 1 - 2.  N = 2 .. MCQ_MAX_N_QUENCH3D and 2 <= Q <= N^3 - 1 (n_queens = 0 means N^2).
 *   2. LOCAL SEARCH L: the mcq_quench3d run with max_passes = 0, passes of its items 3 - 4 until one moves nothing.  A placement that L
 *      returns is a fixed point of L: L moves nothing on it.
 *   3. a call first applies L to the clamped input: energy_in is the recount before it, energy_start is E behind it.  Then it runs
 *      n_hops hops; hop t = 0 .. n_hops - 1 of the call has the GLOBAL index g = first_hop + t.
 *   4. KICK of hop g, with m = kick (1 .. MCQ_MAX_HOP_KICK): for d = 0 .. m - 1 in order, with x1 = word 2 (g m + d) and
 *      x2 = word 2 (g m + d) + 1 of the chain's stream,  n = floor(x1 Q / 2^32)  and  t = floor(x2 N^3 / 2^32), t a cell index
 *      i N^2 + j N + k.  If cell t holds a queen at that moment the draw moves nothing -- queen n's own cell and the cells taken by
 *      earlier draws of this hop included.  Otherwise queen n moves to cell t.  Later draws see earlier ones; a queen may be drawn
 *      twice.  Word w (64-bit) of chain r is
 *        philox4x32-10(counter = (low 32 bits of w / 4, high bits of w / 4, 0, 0), key = (seeds[r], 6))[w % 4]
 *      (key words 0 - 5 are taken by the sweep, the two heat baths, the two tempered sweeps and mcq_hop).
 *   5. L runs on the kicked placement and gives E'.  The hop is ACCEPTED iff E' <= E + slack, E the energy BEFORE the kick: the
 *      placement and E' stay.  Otherwise every queen returns to the cell it held before the kick, and so does E.
 *   6. best_energy, best_hop, best_state, n_accepted, n_improved and energy_hist are those of the mcq_hop rule, items 6 - 7.  n_moves
 *      counts the single-queen moves and n_passes the passes (the last, moveless one of each L too) of every L of the call: that of
 *      item 3 and those of rejected hops too.  n_kicked counts the draws that moved a queen.  All three are int64.
 *   7. a REPEATED input (two queens in one cell after clamping) sets bit 0 of flags (MCQ_HOP3D_REPEATED) and is handed back unmoved:
 *      state_out and best_state are the clamped input, energy_in = energy_start = energy_out = best_energy = the recount (a shared
 *      cell counts as an attacking pair), every counter and best_hop are 0, and energy_hist[0 .. n_hops] all hold the recount.  No
 *      output of the rule is such a placement.
 * Consequences: n_hops = 0 is mcq_quench3d with max_passes = 0.  The state of a chain is its placement plus a hop index and nothing
 * else: a run cut into calls, each fed the state_out of the one before and first_hop carried over, is the unbroken run, because item 3
 * moves nothing on a fixed point of L (the figures of the pieces combine as under mcq_hop; n_passes of a later piece counts the one
 * moveless pass of its item 3 on top).  Chains do not interact, so state_out may be state_in.
 *
 * mcq_hop3d_device keeps a chain in the LDS of one workgroup: 32 dwords, the field (one byte per cell to N = 19, 16 bits beyond), the
 * occupancy bitmap, the queens and the queens from before the kick (16 bits each, each array rounded up to a dword):
 *   bytes = 4 (32 + ceil(N^3 / (4 or 2)) + ceil(N^3 / 32) + 2 ceil(Q / 2)) <= MCQ_MAX_HOP3D_LDS.
 * Every Q = N^2 fits; at N = 32 the largest Q is 23 520.
 */
#define MCQ_MAX_HOP3D_LDS (160 * 1024) /* bytes of LDS a workgroup of mcq_hop3d_device may take */
#define MCQ_HOP3D_REPEATED 1 /* flags bit 0: two queens of the (clamped) input hold the same cell; nothing was moved */
typedef struct mcq_hop3d {
    int32_t N;              /* MCQ_MIN_N .. MCQ_MAX_N_QUENCH3D */
    int32_t n_queens;       /* Q: 2 .. N^3 - 1; 0 = N^2 */
    int64_t n_chains;       /* 1 .. 2^31 - 1 */
    int64_t n_hops;         /* >= 0; 0 = L alone */
    int64_t first_hop;      /* >= 0: the global index of the call's first hop; 2 kick (first_hop + n_hops) < 2^63 */
    int32_t kick;           /* 1 .. MCQ_MAX_HOP_KICK: the draws of one kick */
    int32_t slack;          /* >= 0: a hop may raise E by this much */
    const uint32_t* seeds;  /* [n_chains] */
    const uint8_t* state_in; /* [n_chains][Q][3], final_state layout of full_3d */
    uint8_t* state_out;     /* [n_chains][Q][3]; may be state_in */
    int32_t* energy_in;     /* optional [n_chains]: E of the (clamped) input, recounted */
    int32_t* energy_start;  /* optional [n_chains]: E behind the first L */
    int32_t* energy_out;    /* optional [n_chains]: E of the output */
    int32_t* best_energy;   /* optional [n_chains] */
    int64_t* best_hop;      /* optional [n_chains]: 0 = the placement behind the first L, t + 1 = behind hop t of the call */
    uint8_t* best_state;    /* optional [n_chains][Q][3]; neither state_in nor state_out */
    int64_t* n_accepted;    /* optional [n_chains] */
    int64_t* n_improved;    /* optional [n_chains] */
    int64_t* n_moves;       /* optional [n_chains]: single-queen moves of every L */
    int64_t* n_passes;      /* optional [n_chains]: passes of every L */
    int64_t* n_kicked;      /* optional [n_chains]: draws that moved a queen */
    int32_t* energy_hist;   /* optional [n_chains][hist_stride]: entries 0 .. n_hops */
    int64_t hist_stride;    /* >= n_hops + 1 when energy_hist is given; not read otherwise */
    int32_t* flags;         /* optional [n_chains]: MCQ_HOP3D_* */
} mcq_hop3d;

/* the message of the last error of the calling thread from the two mcq_hop3d_* calls below (they do not set mcq_last_error()) */
const char* mcq_hop3d_last_error(void);
/* Every pointer of `q` is a DEVICE pointer.  One kernel enqueued on `hip_stream`, whatever n_hops is; asynchronous: nothing is
 * copied back and nothing synchronises.  MCQ_EINVAL before any launch: a NULL block, N outside 2 .. 32 (33 .. 64 named as this
 * build's limit), n_queens outside 2 .. N^3 - 1 (0 = N^2), n_chains outside 1 .. 2^31 - 1, a negative n_hops, first_hop or slack, kick
 * outside 1 .. MCQ_MAX_HOP_KICK, 2 kick (first_hop + n_hops) >= 2^63, a NULL seeds, state_in or state_out, hist_stride below
 * n_hops + 1 when energy_hist is given, and any (N, Q) whose chain exceeds MCQ_MAX_HOP3D_LDS (the message names N, Q and the bytes). */
int mcq_hop3d_device(const mcq_hop3d* q, void* hip_stream);
/* The same rule in plain host code over HOST buffers, for every shape (no LDS here), otherwise the same refusals; needs no GPU.  Equal
 * to the kernel bit for bit on every output. */
int mcq_hop3d_host(const mcq_hop3d* q);

/*
 * Tabu search of board placements: every iteration takes the best admissible single-height move of a conflicting column, ALSO when
 * it raises the energy, and forbids the way back for a while (csrc/mcq_tabu.hip) -- NOT a mode of the reference; never a default,
 * like everything above that is labelled so.  The quenches stop on a minimum and the hops fall back onto the one they left; this
 * block walks on from it.  Boards only.  The rule is integer-exact:
 *   1. SETUP.  Every input byte is clamped to N - 1 first; a(c, k) and E are those of the mcq_quench rule, items 1 - 2.
 *      delta(c, k) = a(c, k) - a(c, h(c)), the change of E when column c takes the height k.  Column c is CONFLICTING when
 *      a(c, h(c)) > 0.  No local search is applied to the input; energy_in is its recount.
 *   2. CHAIN STATE: the placement, a stamp T(c, k) >= 0 per column and height, the run's best energy B, and the iteration index.  A
 *      call runs the iterations t = 0 .. n_iters - 1; iteration t has the GLOBAL index g = first_iter + t.  To begin with
 *      T(c, k) = first_iter + tabu_in[c N + k], or 0 everywhere without tabu_in, and B = min(best_floor[r], energy_in), or energy_in
 *      without best_floor.
 *   3. RANDOM WORDS.  Iteration g draws one block (x0, x1, x2, x3) =
 *        philox4x32-10(counter = (low 32 bits of g, high bits of g, 0, 0), key = (seeds[r], 7))
 *      (key words 0 - 6 are taken by the sweep, the two heat baths, the two tempered sweeps, mcq_hop and mcq_hop3d).
 *      o = floor(x0 N^3 / 2^32) is the tie offset, x1 gives the tenure's jitter (item 5), x2 and x3 are unused.
 *   4. CANDIDATES: the (c, k) with c conflicting and k != h(c).  A candidate is TABU when T(c, k) > g.  It is ADMISSIBLE when it is
 *      not tabu, or when E + delta(c, k) < B (aspiration).  The iteration takes the admissible candidate with the lexicographically
 *      smallest (delta, rho), rho = (c N + k - o) mod N^3: of the candidates with the smallest delta the first one at or cyclically
 *      behind a random offset, so ties carry no row-major bias.  With no admissible candidate the iteration moves nothing and counts
 *      in n_stalled; E = 0 is one such case, forever (no column conflicts).
 *   5. THE MOVE of the candidate (c, k), with F the number of conflicting columns BEFORE the move and h_old = h(c):
 *        L = tenure + floor(x1 (tenure_rand + 1) / 2^32) + floor(tenure_conf F / 16)
 *      then T(c, h_old) = g + 1 + L, h(c) = k and E += delta.  (The height left is tabu in the iterations g + 1 .. g + L.)  A move
 *      with E + delta < B sets B, best_iter = t + 1 and the best placement.  best_iter is relative to the call; 0 means the input or an
 *      earlier call.  Counters: n_moves; n_aspired, the moves whose candidate was tabu; n_uphill, the moves with delta > 0;
 *      n_stalled.  All four are int64.
 *   6. OUTPUTS.  energy_hist[r][0 .. n_iters] holds energy_in, then E after each iteration.  energy_out = E and state_out are
 *      those behind the last iteration.  tabu_out[c N + k] = max(0, T(c, k) - (first_iter + n_iters)).  best_energy = B.
 *      best_state is the best placement of THIS call: when no move of the call went below B it is the (clamped) input placement, and
 *      best_energy = B <= energy_in says whether that placement has it.
 * Bounds: tenure 0 .. MCQ_MAX_TABU_TENURE, tenure_rand 0 .. MCQ_MAX_TABU_TENURE_RAND, tenure_conf 0 .. MCQ_MAX_TABU_TENURE_CONF
 * (F <= N^2 <= 1024), so that L <= 8192 + 4095 + 4096 < 2^14, and every tabu_out entry a run writes fits the uint16 of tabu_in /
 * tabu_out (an entry carried from tabu_in only shrinks).  first_iter + n_iters < 2^63.
 * Consequences:
 *   (a) n_iters = 0 is the recount: state_out and best_state are the clamped input, energy_out = energy_in, best_energy = B,
 *       tabu_out = tabu_in, every counter 0.
 *   (b) a run cut into calls is the unbroken run on every output, when each call is fed state_out as state_in, tabu_out as tabu_in,
 *       best_energy as best_floor and first_iter carried over: the four counters add up, the histories join (entry 0 of a later
 *       call repeats the last entry of the one before), and best_iter / best_state are those of the LAST call with best_iter > 0,
 *       its best_iter moved by the iterations before that call.
 *   (c) an improving move (delta < 0) out of a placement with E = B is admissible whatever its stamp, by aspiration.  So whenever
 *       at least one iteration ran behind best_iter (best_iter < n_iters; for best_iter = 0 also B = energy_in), best_state is a
 *       single-move local minimum: mcq_quench moves nothing on it.
 * N = MCQ_MIN_N .. MCQ_MAX_N_QUENCH_PAIRS on the device and in host code alike.  Chains do not interact and a call reads all of a
 * chain's inputs before it writes any of its outputs, so state_out may be state_in and tabu_out may be tabu_in; best_state may be
 * neither state_in nor state_out.
 *
 * mcq_tabu_device keeps a chain in the LDS of one wavefront: the table a(c, k) as bytes in rows of 4 ((NP / 4) | 1) bytes, the stamps
 * as uint16 in rows of 4 ((NP / 2) | 1) bytes, the heights and the best placement, NP = N rounded up to 4, 8, 12, 16, 24 or 32:
 *   bytes = NP^2 (4 ((NP / 4) | 1) + 4 ((NP / 2) | 1) + 2),  108 544 at NP = 32 (one chain per compute unit), <= MCQ_MAX_TABU_LDS.
 */
#define MCQ_MAX_TABU_TENURE 8192
#define MCQ_MAX_TABU_TENURE_RAND 4095
#define MCQ_MAX_TABU_TENURE_CONF 64
#define MCQ_MAX_TABU_LDS (160 * 1024) /* bytes of LDS a workgroup of mcq_tabu_device may take */
typedef struct mcq_tabu {
    int32_t N;              /* MCQ_MIN_N .. MCQ_MAX_N_QUENCH_PAIRS */
    int32_t mode;           /* MCQ_MODE_BOARD; anything else is MCQ_EINVAL */
    int64_t n_chains;       /* 1 .. 2^31 - 1 */
    int64_t n_iters;        /* >= 0; 0 = the recount */
    int64_t first_iter;     /* >= 0: the global index of the call's first iteration; first_iter + n_iters < 2^63 */
    int32_t tenure;         /* 0 .. MCQ_MAX_TABU_TENURE */
    int32_t tenure_rand;    /* 0 .. MCQ_MAX_TABU_TENURE_RAND: the jitter is uniform on 0 .. tenure_rand */
    int32_t tenure_conf;    /* 0 .. MCQ_MAX_TABU_TENURE_CONF: sixteenths of an iteration per conflicting column */
    const uint32_t* seeds;  /* [n_chains] */
    const uint8_t* state_in; /* [n_chains][N*N], final_state layout */
    uint8_t* state_out;     /* [n_chains][N*N]; may be state_in */
    const uint16_t* tabu_in; /* optional [n_chains][N*N*N]: T(c, k) - first_iter, entry c N + k; NULL = nothing is tabu */
    uint16_t* tabu_out;     /* optional [n_chains][N*N*N]; may be tabu_in */
    const int32_t* best_floor; /* optional [n_chains]: the best energy of the calls before */
    int32_t* energy_in;     /* optional [n_chains]: E of the (clamped) input, recounted */
    int32_t* energy_out;    /* optional [n_chains]: E of the output */
    int32_t* best_energy;   /* optional [n_chains]: B */
    int64_t* best_iter;     /* optional [n_chains]: 0 = no move of the call went below B, t + 1 = behind iteration t of the call */
    uint8_t* best_state;    /* optional [n_chains][N*N]; neither state_in nor state_out */
    int64_t* n_moves;       /* optional [n_chains] */
    int64_t* n_aspired;     /* optional [n_chains]: moves whose candidate was tabu */
    int64_t* n_uphill;      /* optional [n_chains]: moves with delta > 0 */
    int64_t* n_stalled;     /* optional [n_chains]: iterations without an admissible candidate */
    int32_t* energy_hist;   /* optional [n_chains][hist_stride]: entries 0 .. n_iters */
    int64_t hist_stride;    /* >= n_iters + 1 when energy_hist is given; not read otherwise */
} mcq_tabu;

/* the message of the last error of the calling thread from the two mcq_tabu_* calls below (they do not set mcq_last_error()) */
const char* mcq_tabu_last_error(void);
/* Every pointer of `q` is a DEVICE pointer.  One kernel enqueued on `hip_stream`, whatever n_iters is; asynchronous: nothing is
 * copied back and nothing synchronises.  MCQ_EINVAL before any launch, each with a message of its own: a NULL block, mode other than
 * board, N out of range, n_chains outside 1 .. 2^31 - 1, a negative n_iters or first_iter, first_iter + n_iters >= 2^63, tenure,
 * tenure_rand or tenure_conf outside their ranges, a NULL seeds, state_in or state_out, hist_stride below n_iters + 1 when energy_hist
 * is given, a best_state that is state_in or state_out, and a chain above MCQ_MAX_TABU_LDS (no N in range is). */
int mcq_tabu_device(const mcq_tabu* q, void* hip_stream);
/* The same rule in plain host code over HOST buffers, same refusals; needs no GPU.  Equal to the kernel bit for bit on every output. */
int mcq_tabu_host(const mcq_tabu* q);

/*
 * Tabu search of full_3d placements: every iteration takes the best admissible move of a conflicting queen to a free cell of the
 * cube, ALSO when it raises the energy, and forbids the cell it left for a while (csrc/mcq_tabu3d.hip) -- NOT a mode of the reference;
 * never a default, like everything above that is labelled so.  mcq_tabu above keeps refusing full_3d: a queen here has N^3 targets
 * and the stamps belong to cells, and this block has its own entry points.  The rule is integer-exact:
 *   1. SETUP.  The placement (Q triples of bytes, 3 Q bytes per chain), the clamping to N - 1, REPEATED, a(q, t) and E are those of
 *      the mcq_quench3d rule, items 1 - 2.  N = 2 .. MCQ_MAX_N_QUENCH3D and 2 <= Q <= N^3 - 1 (n_queens = 0 means N^2).  Queen q is
 *      CONFLICTING when a(q, pos(q)) > 0; a cell is FREE when it holds no queen; delta(q, t) = a(q, t) - a(q, pos(q)), the change of
 *      E when queen q moves to the free cell t.  No local search is applied to the input; energy_in is its recount.
 *   2. CHAIN STATE: the placement, a stamp T(t) >= 0 per cell of the cube, the run's best energy B, and the iteration index.  A
 *      call runs the iterations t = 0 .. n_iters - 1; iteration t has the GLOBAL index g = first_iter + t.  To begin with
 *      T(t) = first_iter + tabu_in[t], or 0 everywhere without tabu_in, t the cell index i N^2 + j N + k, and
 *      B = min(best_floor[r], energy_in), or energy_in without best_floor.
 *   3. RANDOM WORDS.  Iteration g draws one block (x0, x1, x2, x3) =
 *        philox4x32-10(counter = (low 32 bits of g, high bits of g, 0, 0), key = (seeds[r], 8))
 *      (key words 0 - 7 are taken by the sweep, the two heat baths, the two tempered sweeps, mcq_hop, mcq_hop3d and mcq_tabu).
 *      o_q = floor(x0 Q / 2^32) and o_t = floor(x2 N^3 / 2^32) are the tie offsets, x1 gives the tenure's jitter (item 5), x3 is
 *      unused.
 *   4. CANDIDATES: the pairs (q, t) with q conflicting and t free.  A candidate is TABU when T(t) > g: the stamp belongs to the
 *      cell, whichever queen would enter it.  It is ADMISSIBLE when it is not tabu, or when E + delta(q, t) < B (aspiration).  The
 *      iteration takes the admissible candidate with the lexicographically smallest (delta, rho_q, rho_t),
 *      rho_q = (q - o_q) mod Q and rho_t = (t - o_t) mod N^3.  With no admissible candidate the iteration moves nothing and counts
 *      in n_stalled; E = 0 is one such case, forever (no queen conflicts).
 *   5. THE MOVE of the candidate (q, t), with F the number of conflicting queens BEFORE the move and p = pos(q):
 *        L = min(MCQ_MAX_TABU3D_SPAN, tenure + floor(x1 (tenure_rand + 1) / 2^32) + floor(tenure_conf F / 16))
 *      then T(p) = g + 1 + L, pos(q) = t and E += delta.  (The cell left is tabu in the iterations g + 1 .. g + L.)  F may reach
 *      N^3 - 1 here, so L is capped and not the parameters.  A move with E + delta < B sets B, best_iter = t + 1 and the best
 *      placement.  Counters: n_moves; n_aspired, the moves whose candidate was tabu; n_uphill, the moves with delta > 0; n_stalled.
 *      All four are int64.
 *   6. OUTPUTS.  energy_hist, energy_out, state_out, best_energy, best_state and best_iter are exactly as in the mcq_tabu rule,
 *      item 6.  tabu_out[t] = max(0, T(t) - (first_iter + n_iters)).
 *   7. a REPEATED input (two queens in one cell after clamping) sets bit 0 of flags (MCQ_TABU3D_REPEATED) and is handed back
 *      unmoved: state_out and best_state are the clamped input, energy_in = energy_out = best_energy = the recount (a shared cell
 *      counts as an attacking pair; best_floor is not looked at), every counter and best_iter are 0, energy_hist[0 .. n_iters] all
 *      hold the recount, and tabu_out = tabu_in, or zeros without it.  No output of the rule is such a placement.
 * Bounds: tenure, tenure_rand and tenure_conf as under mcq_tabu; L <= MCQ_MAX_TABU3D_SPAN = 2^14 - 1, so that every tabu_out entry a
 * run writes fits the uint16 of tabu_in / tabu_out.  first_iter + n_iters < 2^63.
 * Consequences:
 *   (a) n_iters = 0 is the recount: state_out and best_state are the clamped input, energy_out = energy_in, best_energy = B,
 *       tabu_out = tabu_in, every counter 0.
 *   (b) a run cut into calls is the unbroken run on every output, when each call is fed state_out as state_in, tabu_out as tabu_in,
 *       best_energy as best_floor and first_iter carried over; the figures of the pieces combine as under mcq_tabu (b).
 *   (c) a queen that does not conflict cannot improve, and an improving move out of a placement with E = B is admissible whatever
 *       its stamp, by aspiration.  So whenever at least one iteration ran behind best_iter (best_iter < n_iters; for best_iter = 0
 *       also B = energy_in), mcq_quench3d moves nothing on best_state.
 * Chains do not interact and a call reads all of a chain's inputs before it writes any of its outputs, so state_out may be state_in
 * and tabu_out may be tabu_in; best_state may be neither state_in nor state_out.
 *
 * mcq_tabu3d_device keeps a chain in the LDS of one workgroup: 32 dwords, the stamps (16 bits per cell), the field (one byte per cell
 * to N = 19, 16 bits beyond), the occupancy bitmap and the queens (16 bits each), each array rounded up to a dword:
 *   bytes = 4 (32 + ceil(N^3 / 2) + ceil(N^3 / (4 or 2)) + ceil(N^3 / 32) + ceil(Q / 2)) <= MCQ_MAX_TABU3D_LDS.
 * Every Q = N^2 fits (137 344 bytes at N = 32); at N = 32 the largest Q is 14 272.  mcq_tabu3d_host runs every shape.
 */
#define MCQ_MAX_TABU3D_SPAN 16383 /* 2^14 - 1: the longest tenure L of a move */
#define MCQ_MAX_TABU3D_LDS (160 * 1024) /* bytes of LDS a workgroup of mcq_tabu3d_device may take */
#define MCQ_TABU3D_REPEATED 1 /* flags bit 0: two queens of the (clamped) input hold the same cell; nothing was moved */
typedef struct mcq_tabu3d {
    int32_t N;              /* MCQ_MIN_N .. MCQ_MAX_N_QUENCH3D */
    int32_t n_queens;       /* Q: 2 .. N^3 - 1; 0 = N^2 */
    int64_t n_chains;       /* 1 .. 2^31 - 1 */
    int64_t n_iters;        /* >= 0; 0 = the recount */
    int64_t first_iter;     /* >= 0: the global index of the call's first iteration; first_iter + n_iters < 2^63 */
    int32_t tenure;         /* 0 .. MCQ_MAX_TABU_TENURE */
    int32_t tenure_rand;    /* 0 .. MCQ_MAX_TABU_TENURE_RAND: the jitter is uniform on 0 .. tenure_rand */
    int32_t tenure_conf;    /* 0 .. MCQ_MAX_TABU_TENURE_CONF: sixteenths of an iteration per conflicting queen */
    const uint32_t* seeds;  /* [n_chains] */
    const uint8_t* state_in; /* [n_chains][Q][3], final_state layout of full_3d */
    uint8_t* state_out;     /* [n_chains][Q][3]; may be state_in */
    const uint16_t* tabu_in; /* optional [n_chains][N*N*N]: T(t) - first_iter, entry i N^2 + j N + k; NULL = nothing is tabu */
    uint16_t* tabu_out;     /* optional [n_chains][N*N*N]; may be tabu_in */
    const int32_t* best_floor; /* optional [n_chains]: the best energy of the calls before */
    int32_t* energy_in;     /* optional [n_chains]: E of the (clamped) input, recounted */
    int32_t* energy_out;    /* optional [n_chains]: E of the output */
    int32_t* best_energy;   /* optional [n_chains]: B */
    int64_t* best_iter;     /* optional [n_chains]: 0 = no move of the call went below B, t + 1 = behind iteration t of the call */
    uint8_t* best_state;    /* optional [n_chains][Q][3]; neither state_in nor state_out */
    int64_t* n_moves;       /* optional [n_chains] */
    int64_t* n_aspired;     /* optional [n_chains]: moves whose candidate was tabu */
    int64_t* n_uphill;      /* optional [n_chains]: moves with delta > 0 */
    int64_t* n_stalled;     /* optional [n_chains]: iterations without an admissible candidate */
    int32_t* energy_hist;   /* optional [n_chains][hist_stride]: entries 0 .. n_iters */
    int64_t hist_stride;    /* >= n_iters + 1 when energy_hist is given; not read otherwise */
    int32_t* flags;         /* optional [n_chains]: MCQ_TABU3D_* */
} mcq_tabu3d;

/* the message of the last error of the calling thread from the two mcq_tabu3d_* calls below (they do not set mcq_last_error()) */
const char* mcq_tabu3d_last_error(void);
/* Every pointer of `q` is a DEVICE pointer.  One kernel enqueued on `hip_stream`, whatever n_iters is; asynchronous: nothing is
 * copied back and nothing synchronises.  MCQ_EINVAL before any launch, each with a message of its own: a NULL block, N outside
 * 2 .. 32 (33 .. 64 named as this build's limit), n_queens outside 2 .. N^3 - 1 (0 = N^2), n_chains outside 1 .. 2^31 - 1, a negative
 * n_iters or first_iter, first_iter + n_iters >= 2^63, tenure, tenure_rand or tenure_conf outside their ranges, a NULL seeds, state_in
 * or state_out, hist_stride below n_iters + 1 when energy_hist is given, a best_state that is state_in or state_out, and any (N, Q)
 * whose chain exceeds MCQ_MAX_TABU3D_LDS (the message names N, Q and the bytes). */
int mcq_tabu3d_device(const mcq_tabu3d* q, void* hip_stream);
/* The same rule in plain host code over HOST buffers, for every shape (no LDS here), otherwise the same refusals; needs no GPU.  Equal
 * to the kernel bit for bit on every output. */
int mcq_tabu3d_host(const mcq_tabu3d* q);

/*
 * Path relinking between board placements: walk from a placement A towards a guide G, one column at a time, always the cheapest
 * remaining column, and hand the best placement met on the way to the local search (csrc/mcq_relink.hip) -- NOT a mode of the
 * reference; never a default, like everything above that is labelled so.  Every search above moves one placement; this block
 * combines two.  Boards only.  The rule is integer-exact:
 *   1. SETUP.  Every byte of state_in and of guide_in is clamped to N - 1 first; a(c, k), E and delta(c, k) = a(c, k) - a(c, h(c))
 *      are those of the mcq_tabu rule, item 1.  h is the walking placement and starts as the clamped A = state_in; g is the clamped
 *      guide.  F = {c : h(c) != g(c)} and d0 = |F| at the start (distance_in).  energy_in is the recount of A.
 *   2. WALK.  n_steps = d0 when max_steps = 0, else min(d0, max_steps).  Step t = 0 .. n_steps - 1 draws one block
 *        (x0, x1, x2, x3) = philox4x32-10(counter = (t, low 32 bits of walk, high 32 bits of walk, 0), key = (seeds[r], 9))
 *      (key words 0 - 8 are taken by the sweep, the two heat baths, the two tempered sweeps, mcq_hop, mcq_hop3d, mcq_tabu and
 *      mcq_tabu3d; 9 is this block's).  o = floor(x0 N^2 / 2^32); x1, x2 and x3 are unused.  Of the columns c in F the step takes
 *      the one with the lexicographically smallest (delta(c, g(c)), (c - o) mod N^2); then h(c) = g(c), E += delta and c leaves F.
 *      A rise is taken like a fall.  walk >= 0 is a caller's index, so that repeated walks from the same seeds take different tie
 *      orders.
 *   3. CANDIDATES.  The placement behind step t (t counted from 1 here) is at distance t from A and d0 - t from G.  It is a CANDIDATE
 *      when t >= max(1, min_dist) and d0 - t >= min_dist.  P* is the candidate with the smallest E, the earliest on ties:
 *      path_best_step = its t, path_best_energy = its E.  With no candidate P* is the clamped A, path_best_step = 0 and
 *      path_best_energy = energy_in.  P* need not lie below A.  path_best_state = P*.  path_max_energy is the largest entry of the
 *      walk's energies, energy_in included.
 *   4. LOCAL SEARCH.  L of the mcq_hop rule, item 2, by local_search (MCQ_HOP_SINGLE or MCQ_HOP_PAIRS), runs on P*: state_out and
 *      energy_out are the placement and E behind it, n_moves and n_pair_moves its single and pair moves (int64).
 *   5. HISTORY.  energy_hist[r][0 .. W], W = max_steps, or N^2 when that is 0: entry 0 is energy_in, entry t is E behind step t, and
 *      the entries behind n_steps repeat the last one.  hist_stride >= W + 1 when energy_hist is given.
 * Consequences:
 *   (a) with d0 = 0 the call is L alone: state_out, energy_out, n_moves and n_pair_moves are those of mcq_quench_pairs with
 *       max_rounds = 0 (MCQ_HOP_PAIRS) or of mcq_quench with max_passes = 0 (MCQ_HOP_SINGLE).
 *   (b) with max_steps = 0 the walk ends on g: entry d0 of the history is the energy_in of a call whose state_in is the guide.
 *   (c) state_out is a fixed point of L.
 *   (d) path_best_energy = E of path_best_state, and energy_out <= path_best_energy.
 * N = MCQ_MIN_N .. MCQ_MAX_N_QUENCH_PAIRS on the device and in host code alike.  Chains do not interact and a call reads all of a
 * chain's inputs before it writes any of its outputs, so state_out may be state_in; it may not be guide_in (the guides stay the
 * caller's: a pool that relinks each slot with a rolled view of itself reads them again).  path_best_state is none of state_in,
 * guide_in and state_out.
 *
 * mcq_relink_device keeps a chain in the LDS of one wavefront: the table a(c, k) as bytes in rows of 4 ((NP / 4) | 1) bytes, the
 * heights h, g and P* (a byte per column each) and, under MCQ_HOP_PAIRS, the two mask words per column of the pair scan, NP = N
 * rounded up to 4, 8, 12, 16, 24 or 32:
 *   bytes = NP^2 (4 ((NP / 4) | 1) + 3), and 8 NP^2 more under MCQ_HOP_PAIRS:  48 128 at NP = 32, <= MCQ_MAX_RELINK_LDS.
 */
#define MCQ_MAX_RELINK_LDS (160 * 1024) /* bytes of LDS a workgroup of mcq_relink_device may take */
typedef struct mcq_relink {
    int32_t N;              /* MCQ_MIN_N .. MCQ_MAX_N_QUENCH_PAIRS */
    int32_t mode;           /* MCQ_MODE_BOARD; anything else is MCQ_EINVAL */
    int64_t n_chains;       /* 1 .. 2^31 - 1 */
    int32_t max_steps;      /* 0 .. N^2; 0 = the whole way to the guide */
    int32_t min_dist;       /* 0 .. N^2: a candidate is at least this far from the guide, and max(1, min_dist) from A */
    int32_t local_search;   /* MCQ_HOP_SINGLE or MCQ_HOP_PAIRS */
    int64_t walk;           /* >= 0: the caller's index of the walk, counter words 1 and 2 of the tie offsets' blocks */
    const uint32_t* seeds;  /* [n_chains] */
    const uint8_t* state_in; /* [n_chains][N*N], final_state layout: A */
    const uint8_t* guide_in; /* [n_chains][N*N]: G */
    uint8_t* state_out;     /* [n_chains][N*N]; may be state_in, may not be guide_in */
    uint8_t* path_best_state; /* optional [n_chains][N*N]: P*; none of state_in, guide_in, state_out */
    int32_t* distance_in;   /* optional [n_chains]: d0 */
    int32_t* n_steps;       /* optional [n_chains] */
    int32_t* path_best_step; /* optional [n_chains]: 0 = no candidate (P* = A), else t of P* */
    int32_t* energy_in;     /* optional [n_chains]: E of the (clamped) A, recounted */
    int32_t* path_best_energy; /* optional [n_chains]: E of P* */
    int32_t* path_max_energy; /* optional [n_chains]: the largest energy of the walk, energy_in included */
    int32_t* energy_out;    /* optional [n_chains]: E of the output */
    int64_t* n_moves;       /* optional [n_chains]: single moves of L */
    int64_t* n_pair_moves;  /* optional [n_chains]: pair moves of L (0 under MCQ_HOP_SINGLE) */
    int32_t* energy_hist;   /* optional [n_chains][hist_stride]: entries 0 .. W, W = max_steps or N^2 */
    int64_t hist_stride;    /* >= W + 1 when energy_hist is given; not read otherwise */
} mcq_relink;

/* the message of the last error of the calling thread from the two mcq_relink_* calls below (they do not set mcq_last_error()) */
const char* mcq_relink_last_error(void);
/* Every pointer of `q` is a DEVICE pointer.  One kernel enqueued on `hip_stream`, whatever the distances are; asynchronous: nothing
 * is copied back and nothing synchronises.  MCQ_EINVAL before any launch, each with a message of its own: a NULL block, mode other
 * than board, N out of range, n_chains outside 1 .. 2^31 - 1, max_steps or min_dist outside 0 .. N^2, a local_search that is neither
 * value, a negative walk, a NULL seeds, state_in, guide_in or state_out, a state_out that is guide_in, a path_best_state that is
 * state_in, guide_in or state_out, hist_stride below W + 1 when energy_hist is given, and a chain above MCQ_MAX_RELINK_LDS (no N in
 * range is). */
int mcq_relink_device(const mcq_relink* q, void* hip_stream);
/* The same rule in plain host code over HOST buffers, same refusals; needs no GPU.  Equal to the kernel bit for bit on every output. */
int mcq_relink_host(const mcq_relink* q);

/*
 * Path relinking between full_3d placements: walk from a placement A towards a guide G, one queen at a time, always the cheapest
 * remaining (queen, cell) pair, and hand the best placement met on the way to the local search (csrc/mcq_relink3d.hip) -- NOT a mode
 * of the reference; never a default, like everything above that is labelled so.  mcq_relink above keeps refusing full_3d: a guide
 * here is a set of cells, a step chooses the queen AND its target, and this block has its own entry points.  The rule is
 * integer-exact:
 *   1. SETUP.  state_in (A) and guide_in (G) are Q triples of bytes per chain (3 Q bytes each); the clamping to N - 1, REPEATED,
 *      a(q, t) and E are those of the mcq_quench3d rule, items 1 - 2.  N = 2 .. MCQ_MAX_N_QUENCH3D and 2 <= Q <= N^3 - 1 (n_queens = 0
 *      means N^2).  h is the walking placement and starts as the clamped A.  The guide is a SET OF CELLS, cells(G): the order of its
 *      queens means nothing.  M = {q : pos(q) not in cells(G)} are the moving queens, T = cells(G) \ cells(h) the open targets;
 *      |M| = |T| = d0 at the start (distance_in).  energy_in is the recount of A.
 *   2. WALK.  n_steps = d0 when max_steps = 0, else min(d0, max_steps).  Step t = 0 .. n_steps - 1 draws one block
 *        (x0, x1, x2, x3) = philox4x32-10(counter = (t, low 32 bits of walk, high 32 bits of walk, 0), key = (seeds[r], 10))
 *      (key words 0 - 9 are taken by the sweep, the two heat baths, the two tempered sweeps, mcq_hop, mcq_hop3d, mcq_tabu, mcq_tabu3d
 *      and mcq_relink; 10 is this block's).  o_q = floor(x0 Q / 2^32) and o_t = floor(x1 N^3 / 2^32) are the tie offsets; x2 and x3
 *      are unused.  Of all pairs (q in M, c in T) the step takes the one with the lexicographically smallest
 *        (delta(q, c), (q - o_q) mod Q, (c - o_t) mod N^3),   delta(q, c) = a(q, c) - a(q, pos(q)),
 *      c the cell index i N^2 + j N + k.  With S the field of the whole placement (S(t) = the queens that hold or attack t),
 *      delta(q, c) = S(c) - [pos(q) attacks c] - (S(pos(q)) - 1).  Queen q moves to c, E += delta, q leaves M and c leaves T.  A rise
 *      is taken like a fall.  Queens keep the indices they have in A, so state_out is in A's order.  walk >= 0 is a caller's index,
 *      as under mcq_relink.
 *   3. CANDIDATES.  The placement behind step t (t counted from 1 here) is at distance t from A and d0 - t from G.  It is a CANDIDATE
 *      when t >= max(1, min_dist) and d0 - t >= min_dist.  P* is the candidate with the smallest E, the earliest on ties:
 *      path_best_step = its t, path_best_energy = its E.  With no candidate P* is the clamped A, path_best_step = 0 and
 *      path_best_energy = energy_in.  P* need not lie below A.  path_best_state = P*.  path_max_energy is the largest entry of the
 *      walk's energies, energy_in included.
 *   4. LOCAL SEARCH.  L of the mcq_hop3d rule, item 2 (mcq_quench3d with max_passes = 0), runs on P*: state_out and energy_out are
 *      the placement and E behind it, n_moves and n_passes its moves and passes (int64; the last, moveless pass counts).
 *   5. HISTORY.  energy_hist[r][0 .. W], W = max_steps, or Q when that is 0: entry 0 is energy_in, entry t is E behind step t, and
 *      the entries behind n_steps repeat the last one.  hist_stride >= W + 1 when energy_hist is given.
 *   6. REPEATED INPUTS.  A repeated A (two queens in one cell after clamping) sets bit 0 of flags (MCQ_RELINK3D_REPEATED), a repeated
 *      G sets bit 1 (MCQ_RELINK3D_GUIDE_REPEATED).  Either hands the chain back unmoved: state_out = path_best_state = the clamped A;
 *      energy_in = path_best_energy = path_max_energy = energy_out = the pairwise recount of A (a shared cell counts as an attacking
 *      pair); distance_in, n_steps, path_best_step, n_moves and n_passes are 0; energy_hist[0 .. W] all hold the recount.
 * Consequences:
 *   (a) with cells(G) = cells(A), in any order of the guide's queens, d0 = 0 and the call is mcq_quench3d with max_passes = 0 alone.
 *   (b) with max_steps = 0 the walk ends on the guide's cells: entry d0 of the history is the energy of G.
 *   (c) state_out is a fixed point of L.
 *   (d) path_best_energy = E of path_best_state, and energy_out <= path_best_energy.
 *   (e) permuting the guide's queens changes no output.
 * Chains do not interact and a call reads all of a chain's inputs before it writes any of its outputs, so state_out may be state_in;
 * it may not be guide_in; path_best_state is none of state_in, guide_in and state_out.
 *
 * mcq_relink3d_device keeps a chain in the LDS of one workgroup: 32 dwords, the guide's bitmap, the field (one byte per cell to
 * N = 19, 16 bits beyond), the occupancy bitmap, the queens and P* (16 bits a queen each) and the lists of M and T (16 bits an entry,
 * D = min(Q, N^3 - Q) entries each: d0 is at most the queens and at most the free cells), each array rounded up to a dword:
 *   bytes = 4 (32 + 2 ceil(N^3 / 32) + ceil(N^3 / (4 or 2)) + 2 ceil(Q / 2) + 2 ceil(D / 2)) <= MCQ_MAX_RELINK3D_LDS.
 * Every Q = N^2 fits (3 440 bytes at N = 12, 82 048 at N = 32); every Q fits up to N = 29; at N = 32 the largest Q is 11 248.
 * mcq_relink3d_host runs every shape.
 */
#define MCQ_MAX_RELINK3D_LDS (160 * 1024) /* bytes of LDS a workgroup of mcq_relink3d_device may take */
#define MCQ_RELINK3D_REPEATED 1 /* flags bit 0: two queens of the (clamped) state_in hold the same cell; nothing was moved */
#define MCQ_RELINK3D_GUIDE_REPEATED 2 /* flags bit 1: two queens of the (clamped) guide_in hold the same cell; nothing was moved */
typedef struct mcq_relink3d {
    int32_t N;              /* MCQ_MIN_N .. MCQ_MAX_N_QUENCH3D */
    int32_t n_queens;       /* Q: 2 .. N^3 - 1; 0 = N^2 */
    int64_t n_chains;       /* 1 .. 2^31 - 1 */
    int32_t max_steps;      /* 0 .. Q; 0 = the whole way to the guide */
    int32_t min_dist;       /* 0 .. Q: a candidate is at least this far from the guide, and max(1, min_dist) from A */
    int64_t walk;           /* >= 0: the caller's index of the walk, counter words 1 and 2 of the tie offsets' blocks */
    const uint32_t* seeds;  /* [n_chains] */
    const uint8_t* state_in; /* [n_chains][Q][3], final_state layout of full_3d: A */
    const uint8_t* guide_in; /* [n_chains][Q][3]: G, read as a set of cells */
    uint8_t* state_out;     /* [n_chains][Q][3]; may be state_in, may not be guide_in */
    uint8_t* path_best_state; /* optional [n_chains][Q][3]: P*; none of state_in, guide_in, state_out */
    int32_t* distance_in;   /* optional [n_chains]: d0 */
    int32_t* n_steps;       /* optional [n_chains] */
    int32_t* path_best_step; /* optional [n_chains]: 0 = no candidate (P* = A), else t of P* */
    int32_t* energy_in;     /* optional [n_chains]: E of the (clamped) A, recounted */
    int32_t* path_best_energy; /* optional [n_chains]: E of P* */
    int32_t* path_max_energy; /* optional [n_chains]: the largest energy of the walk, energy_in included */
    int32_t* energy_out;    /* optional [n_chains]: E of the output */
    int64_t* n_moves;       /* optional [n_chains]: moves of L */
    int64_t* n_passes;      /* optional [n_chains]: passes of L, the moveless one included */
    int32_t* energy_hist;   /* optional [n_chains][hist_stride]: entries 0 .. W, W = max_steps or Q */
    int64_t hist_stride;    /* >= W + 1 when energy_hist is given; not read otherwise */
    int32_t* flags;         /* optional [n_chains]: MCQ_RELINK3D_* */
} mcq_relink3d;

/* the message of the last error of the calling thread from the two mcq_relink3d_* calls below (they do not set mcq_last_error()) */
const char* mcq_relink3d_last_error(void);
/* Every pointer of `q` is a DEVICE pointer.  One kernel enqueued on `hip_stream`, whatever the distances are; asynchronous: nothing
 * is copied back and nothing synchronises.  MCQ_EINVAL before any launch, each with a message of its own: a NULL block, N outside
 * 2 .. 32 (33 .. 64 named as this build's limit), n_queens outside 2 .. N^3 - 1 (0 = N^2), n_chains outside 1 .. 2^31 - 1, max_steps
 * or min_dist outside 0 .. Q, a negative walk, a NULL seeds, state_in, guide_in or state_out, a state_out that is guide_in, a
 * path_best_state that is state_in, guide_in or state_out, hist_stride below W + 1 when energy_hist is given, and any (N, Q) whose
 * chain exceeds MCQ_MAX_RELINK3D_LDS (the message names N, Q and the bytes). */
int mcq_relink3d_device(const mcq_relink3d* q, void* hip_stream);
/* The same rule in plain host code over HOST buffers, for every shape (no LDS here), otherwise the same refusals; needs no GPU.  Equal
 * to the kernel bit for bit on every output. */
int mcq_relink3d_host(const mcq_relink3d* q);

/*
 * The n-fold way (Bortz, Kalos, Lebowitz): a rejection-free form of the Metropolis dynamics of board placements (csrc/mcq_nfold.hip)
 * -- NOT a mode of the reference; never a default, like everything above that is labelled so.  The reference proposes one random
 * column and one random height per step and rejects most of them; this block holds the acceptance weight of all N^2 (N - 1) moves of
 * a board, draws the next ACCEPTED move in proportion to its weight and advances the clock by the time the Metropolis chain would
 * have spent rejecting.  The process is the Metropolis chain with the same stationary distribution and the same time axis, counted
 * in Metropolis steps.  Boards only, N = MCQ_MIN_N .. MCQ_MAX_N_QUENCH_PAIRS.  The rule is integer-exact:
 *   1. INPUT.  Every byte of state_in is clamped to N - 1; a(c, k) and E are those of the mcq_quench rule.  energy_in is the recount.
 *   2. SEGMENTS.  A call runs n_segs segments of seg_steps Metropolis steps each, 1 <= seg_steps <= 2^31.  Segment s = 0 .. n_segs - 1
 *      has the global index g = first_seg + s and the weight row T_s = table[s][0 .. table_len - 1], uint32, 1 <= table_len = D <=
 *      MCQ_MAX_NFOLD_TABLE (a difference never exceeds 4 (N - 1) = 124); every entry is <= 2^24.  beta is constant inside a segment:
 *      T_s[d] = floor(2^24 exp(-beta_s d)) is what the Python side builds, but the rows are the caller's.
 *   3. WEIGHTS.  For a column c and a height k != h(c):  d = a(c, k) - a(c, h(c)),  w(c, k) = T_s[min(max(d, 0), D - 1)],
 *      R(c) = sum over k of w(c, k) in uint32, W = sum over c of R(c) in uint64; W <= M 2^24 < 2^40 with M = N^2 (N - 1).
 *      W / (M 2^24) is the probability that one Metropolis step of the reference is accepted.
 *   4. TIME is counted in units of 2^-MCQ_NFOLD_TIME_BITS = 2^-12 step.  A chain holds `need`, a uint64: the hazard left until its
 *      next event.  At the start of a segment left = seg_steps << 12.  Repeat, with tau = max(1, floor((need << 12) / W)):
 *        if W > 0 and tau <= left:  left -= tau, the event fires (items 5 and 6) and need is drawn anew;
 *        otherwise:  need -= floor(left W / 2^12) (the product fits 64 bits whenever this branch is taken; W = 0 leaves need as it
 *        is), and the segment ends.
 *      So a strict minimum under a row with T[d > 0] = 0 sleeps, and its need is kept.
 *   5. DRAWS.  One Philox block per event: block e of chain r is
 *        (x0, x1, x2, x3) = philox4x32-10(counter = (low 32 bits of e, high 32 bits of e, 0, 0), key = (seeds[r], 11))
 *      (key words 0 - 10 are taken by the sweep, the two heat baths, the two tempered sweeps, mcq_hop, mcq_hop3d, mcq_tabu,
 *      mcq_tabu3d, mcq_relink and mcq_relink3d; 11 is this block's).  e is the chain's own event counter; it starts at events_in[r],
 *      or at 0 when events_in is NULL.  x2 of block e gives the need of the wait that ENDS in event e:
 *        need = M l(x2),   l(x) = z clock_ln2 + clock_table[y],
 *      z = the number of leading zero bits of x (32 for x = 0) and y = bits 30 .. 23 of x << z: the 8 bits below the leading one
 *      bit, zeros where x has none; y = 0 for x = 0.  clock_table is uint32[256] with every entry <= 2^26 and clock_ln2 <= 2^24, so
 *      need < 2^45.  With clock_ln2 = round(2^24 ln 2) and clock_table[i] = round(-2^24 ln((256 + i + 1/2) / 512)), l / 2^24 is an
 *      exponential variate of mean 1 to about 1e-6; clock_ln2 = 0 and a table of 2^24 give the deterministic expected waiting time.
 *      A chain without need_in draws its first need from block events_in[r]; a need_in entry is < 2^45, like a drawn one.
 *      x0 and x1 of block e choose the move of event e:  X = x0 2^32 + x1,  U = floor(X W / 2^64) from the full 128-bit product, and
 *      the move is the first (c, k) in the order c ascending, k ascending, k != h(c), whose inclusive prefix sum of w exceeds U.
 *      x3 is unused.
 *   6. EVENT.  h(c) = k, E += d, e += 1; n_uphill counts the events with d > 0, n_flat those with d = 0.  The best values follow a
 *      strictly lower E at every event: best_energy, best_state and
 *        best_step = s seg_steps + (((seg_steps << 12) - left) >> 12),
 *      relative to the call, `left` read behind the event's tau.  They start as energy_in, the clamped input and 0.
 *      energy_hist[r][0 .. n_segs] (optional) holds the recount and then E at the end of every segment.
 *   7. OUTPUTS.  state_out, best_state; energy_in, energy_out, best_energy; best_step, events_out (e behind the call), n_uphill,
 *      n_flat; need_out; weight_out = W of the output under the call's last row (0 when n_segs = 0): the Metropolis acceptance rate
 *      there times M 2^24.
 *   8. CUTTING A RUN.  A run cut at a segment boundary is the unbroken run: the caller carries state_out -> state_in, need_out ->
 *      need_in, events_out -> events_in and first_seg, and hands each piece its rows.  n_segs = 0 is a recount and a copy.
 * Chains do not interact and a call reads all of a chain's inputs before it writes any of its outputs, so state_out may be state_in.
 *
 * mcq_nfold_device keeps a chain in the LDS of one wavefront: the table a(c, k) in the layout of csrc/mcq_table.h, the heights and
 * the best placement (a byte per column each), R(c) (a dword per column, padded to an odd stride per lane) and the staged row T_s.
 */
#define MCQ_MAX_NFOLD_TABLE 128 /* the largest table_len of mcq_nfold: 4 (MCQ_MAX_N_QUENCH_PAIRS - 1) = 124 is the largest difference */
#define MCQ_NFOLD_TIME_BITS 12  /* time is counted in units of 2^-12 Metropolis step */
#define MCQ_NFOLD_WEIGHT_BITS 24 /* no entry of a weight row exceeds 2^24 */
#define MCQ_NFOLD_CLOCK_BITS 26 /* no entry of clock_table exceeds 2^26; clock_ln2 <= 2^24 */
#define MCQ_NFOLD_NEED_BITS 45  /* need < 2^45 */
#define MCQ_NFOLD_STEP_BITS 50  /* (first_seg + n_segs) seg_steps < 2^50 */
typedef struct mcq_nfold {
    int32_t N;              /* MCQ_MIN_N .. MCQ_MAX_N_QUENCH_PAIRS */
    int32_t mode;           /* MCQ_MODE_BOARD; anything else is MCQ_EINVAL */
    int64_t n_chains;       /* 1 .. 2^31 - 1 */
    int64_t n_segs;         /* >= 0; 0 = a recount and a copy */
    int64_t first_seg;      /* >= 0: the global index of the call's first segment */
    int64_t seg_steps;      /* 1 .. 2^31 Metropolis steps per segment; (first_seg + n_segs) seg_steps < 2^50 */
    const uint32_t* seeds;  /* [n_chains] */
    const uint32_t* table;  /* [n_segs][table_len]: the weight rows, every entry <= 2^24; may be NULL when n_segs = 0 */
    int64_t table_len;      /* D: 1 .. MCQ_MAX_NFOLD_TABLE */
    const uint32_t* clock_table; /* [256]: every entry <= 2^26 */
    int64_t clock_ln2;      /* 0 .. 2^24 */
    const uint64_t* need_in; /* optional [n_chains]: the hazard left from the piece before, each < 2^45; NULL: drawn from block events_in[r] */
    const int64_t* events_in; /* optional [n_chains]: the event counters the chains start at, each >= 0; NULL: 0 */
    const uint8_t* state_in; /* [n_chains][N*N], final_state layout */
    uint8_t* state_out;     /* [n_chains][N*N]; may be state_in */
    uint8_t* best_state;    /* optional [n_chains][N*N]; neither state_in nor state_out */
    int32_t* energy_in;     /* optional [n_chains]: E of the (clamped) input, recounted */
    int32_t* energy_out;    /* optional [n_chains] */
    int32_t* best_energy;   /* optional [n_chains] */
    int64_t* best_step;     /* optional [n_chains]: the Metropolis step of the call at which best_energy was first reached; 0 = the input */
    int64_t* events_out;    /* optional [n_chains]: the event counter behind the call */
    int64_t* n_uphill;      /* optional [n_chains]: events of this call with d > 0 */
    int64_t* n_flat;        /* optional [n_chains]: events of this call with d = 0 */
    uint64_t* need_out;     /* optional [n_chains] */
    uint64_t* weight_out;   /* optional [n_chains]: W of the output under the last row; 0 when n_segs = 0 */
    int32_t* energy_hist;   /* optional [n_chains][hist_stride]: entries 0 .. n_segs */
    int64_t hist_stride;    /* >= n_segs + 1 when energy_hist is given; not read otherwise */
} mcq_nfold;

/* the message of the last error of the calling thread from the two mcq_nfold_* calls below (they do not set mcq_last_error()) */
const char* mcq_nfold_last_error(void);
/* Every pointer of `q` is a DEVICE pointer.  One kernel enqueued on `hip_stream`, whatever n_segs is; asynchronous: nothing is copied
 * back and nothing synchronises.  MCQ_EINVAL before any launch, each with a message of its own: a NULL block, mode other than board,
 * N out of range, n_chains outside 1 .. 2^31 - 1, a negative n_segs or first_seg, seg_steps outside 1 .. 2^31,
 * (first_seg + n_segs) seg_steps >= 2^50, table_len outside 1 .. MCQ_MAX_NFOLD_TABLE, clock_ln2 outside 0 .. 2^24, a NULL seeds,
 * state_in, state_out or clock_table, a NULL table with n_segs > 0, a best_state that is state_in or state_out, and hist_stride below n_segs + 1
 * when energy_hist is given.  The entries of the tables, of need_in and of events_in cannot be looked at here: they are the caller's. */
int mcq_nfold_device(const mcq_nfold* q, void* hip_stream);
/* The same rule in plain host code over HOST buffers, same refusals; needs no GPU.  It also reads the tables and refuses a weight above
 * 2^24, a clock_table entry above 2^26, a need_in entry >= 2^45 and a negative events_in entry.  Equal to the kernel bit for bit on
 * every output. */
int mcq_nfold_host(const mcq_nfold* q);

/*
 * The n-fold way for full_3d placements: the rejection-free form of the Metropolis dynamics of the reference's default move
 * (csrc/mcq_nfold3d.hip) -- NOT a mode of the reference; never a default, like everything above that is labelled so.  mcq_nfold above
 * keeps refusing full_3d: a queen here has N^3 - Q targets, and this block has its own entry points.  The reference draws a uniform
 * queen and a uniform cell among the N^3 - Q cells that hold no queen (it redraws occupied cells before the step counts), so a step
 * proposes one of M = Q (N^3 - Q) moves uniformly; this block holds the acceptance weight of all of them.  The rule is integer-exact;
 * items 2, 4, 5, 7 and 8 of the mcq_nfold rule carry over word for word except where stated here:
 *   1. INPUT.  state_in is uint8[n_chains][3 Q], every byte clamped to N - 1; N = MCQ_MIN_N .. MCQ_MAX_N_QUENCH3D and
 *      2 <= Q <= N^3 - 1 (n_queens = 0 means N^2).  S(t) is the number of queens that hold or attack cell t (csrc/mcq_field.h), the
 *      attack and E are those of the mcq_quench3d rule; energy_in is the recount.  A REPEATED placement (two queens in one cell after
 *      clamping) sets bit 0 of flags (MCQ_NFOLD3D_REPEATED) and is handed back unmoved: state_out and best_state are the clamped input,
 *      energy_in = energy_out = best_energy = the pairwise recount (a shared cell counts as an attacking pair), energy_hist holds it
 *      throughout, events_out is the start counter, need_out is need_in or, without one, the need drawn from block events_in[r],
 *      weight_out, best_step, n_uphill and n_flat are 0.
 *   2. WEIGHTS.  For queen q at p and a cell t that holds no queen:  a(q, t) = S(t) - [p attacks t],  c_q = S(p) - 1,
 *      d = a(q, t) - c_q,  w(q, t) = T_s[min(max(d, 0), D - 1)].  Cells that hold a queen carry no weight.  R(q) = sum over t of
 *      w(q, t) in uint64 (it reaches 2^39), W = sum over q of R(q) <= M 2^24 < 2^52.  1 <= D <= MCQ_MAX_NFOLD3D_TABLE = 512 (the
 *      largest difference is 13 (N - 1) = 403); every entry is <= 2^24.  W / (M 2^24) is the probability that one Metropolis step of
 *      the reference is accepted.
 *   3. TIME.  need = M l(x2) < 2^58 (MCQ_NFOLD3D_NEED_BITS), so need << 12 no longer fits 64 bits and tau is stated as the exact
 *      quotient:  tau = max(1, floor(need 2^12 / W)).  (64-bit arithmetic forms it as q1 = need div W, r1 = need mod W,
 *      tau0 = q1 2^12 + floor(r1 2^12 / W) with r1 2^12 < 2^64; q1 >= 2^32 means tau > left with nothing more to compute.)  When
 *      W > 0 and tau <= left the event fires and left -= tau; otherwise need -= floor(left W / 2^12), a 96-bit product whose quotient
 *      is at most need (W = 0 leaves need as it is), and the segment ends.
 *   4. DRAWS.  Block e of chain r is philox4x32-10(counter = (low 32 bits of e, high 32 bits of e, 0, 0), key = (seeds[r], 12))
 *      (key words 0 - 11 are taken by the sweep, the two heat baths, the two tempered sweeps, mcq_hop, mcq_hop3d, mcq_tabu, mcq_tabu3d,
 *      mcq_relink, mcq_relink3d and mcq_nfold; 12 is this block's).  x2 gives the need as under mcq_nfold, with this M.
 *      U = floor(X W / 2^64), X = x0 2^32 + x1, and the move is the first (q, t) whose inclusive prefix sum of w exceeds U, in the
 *      order q ascending, then cell index (i N + j) N + k ascending over the cells that hold no queen.  x3 is unused.
 *   5. EVENT.  Queen q moves to t, E += d, e += 1; the counters, best_energy, best_state and best_step are as under mcq_nfold.
 *   6. OUTPUTS.  Those of mcq_nfold, and flags.
 *   7. CUTTING A RUN.  As under mcq_nfold: a run cut at a segment boundary is the unbroken run; n_segs = 0 is a recount and a copy.
 * Chains do not interact and a call reads all of a chain's inputs before it writes any of its outputs, so state_out may be state_in;
 * best_state may be neither state_in nor state_out.
 *
 * mcq_nfold3d_device keeps a chain in the LDS of one workgroup: 2 376 dwords (reductions, the row T_s, the clock table, a histogram
 * of S over the free cells and a sum per c_q), R(q) (a uint64 per queen), the field (one byte per cell to N = 19, 16 bits beyond),
 * the occupancy bitmap and the queens (16 bits each), each array rounded up to a dword:
 *   bytes = 4 (2376 + 2 Q + ceil(N^3 / (4 or 2)) + ceil(N^3 / 32) + ceil(Q / 2)) <= MCQ_MAX_NFOLD3D_LDS.
 * Every Q = N^2 fits (89 376 bytes at N = 32); at N = 32 the largest Q is 8 470.  mcq_nfold3d_host runs every shape.
 */
#define MCQ_MAX_NFOLD3D_TABLE 512 /* the largest table_len of mcq_nfold3d, as MCQ_MAX_HEATBATH_TABLE: 13 (MCQ_MAX_N_QUENCH3D - 1) = 403 is the largest difference */
#define MCQ_NFOLD3D_NEED_BITS 58  /* need < 2^58 */
#define MCQ_MAX_NFOLD3D_LDS (160 * 1024) /* bytes of LDS a workgroup of mcq_nfold3d_device may take */
#define MCQ_NFOLD3D_REPEATED 1 /* flags bit 0: two queens of the (clamped) input hold the same cell; nothing was moved */
typedef struct mcq_nfold3d {
    int32_t N;              /* MCQ_MIN_N .. MCQ_MAX_N_QUENCH3D */
    int32_t mode;           /* MCQ_MODE_FULL3D; anything else is MCQ_EINVAL (boards are mcq_nfold's) */
    int32_t n_queens;       /* Q: 2 .. N^3 - 1; 0 = N^2 */
    int64_t n_chains;       /* 1 .. 2^31 - 1 */
    int64_t n_segs;         /* >= 0; 0 = a recount and a copy */
    int64_t first_seg;      /* >= 0: the global index of the call's first segment */
    int64_t seg_steps;      /* 1 .. 2^31 Metropolis steps per segment; (first_seg + n_segs) seg_steps < 2^50 */
    const uint32_t* seeds;  /* [n_chains] */
    const uint32_t* table;  /* [n_segs][table_len]: the weight rows, every entry <= 2^24; may be NULL when n_segs = 0 */
    int64_t table_len;      /* D: 1 .. MCQ_MAX_NFOLD3D_TABLE */
    const uint32_t* clock_table; /* [256]: every entry <= 2^26 */
    int64_t clock_ln2;      /* 0 .. 2^24 */
    const uint64_t* need_in; /* optional [n_chains]: the hazard left from the piece before, each < 2^58; NULL: drawn from block events_in[r] */
    const int64_t* events_in; /* optional [n_chains]: the event counters the chains start at, each >= 0; NULL: 0 */
    const uint8_t* state_in; /* [n_chains][Q][3], final_state layout of full_3d */
    uint8_t* state_out;     /* [n_chains][Q][3]; may be state_in */
    uint8_t* best_state;    /* optional [n_chains][Q][3]; neither state_in nor state_out */
    int32_t* energy_in;     /* optional [n_chains]: E of the (clamped) input, recounted */
    int32_t* energy_out;    /* optional [n_chains] */
    int32_t* best_energy;   /* optional [n_chains] */
    int64_t* best_step;     /* optional [n_chains]: the Metropolis step of the call at which best_energy was first reached; 0 = the input */
    int64_t* events_out;    /* optional [n_chains]: the event counter behind the call */
    int64_t* n_uphill;      /* optional [n_chains]: events of this call with d > 0 */
    int64_t* n_flat;        /* optional [n_chains]: events of this call with d = 0 */
    uint64_t* need_out;     /* optional [n_chains] */
    uint64_t* weight_out;   /* optional [n_chains]: W of the output under the last row; 0 when n_segs = 0 */
    int32_t* energy_hist;   /* optional [n_chains][hist_stride]: entries 0 .. n_segs */
    int64_t hist_stride;    /* >= n_segs + 1 when energy_hist is given; not read otherwise */
    int32_t* flags;         /* optional [n_chains]: MCQ_NFOLD3D_* */
} mcq_nfold3d;

/* the message of the last error of the calling thread from the two mcq_nfold3d_* calls below (they do not set mcq_last_error()) */
const char* mcq_nfold3d_last_error(void);
/* Every pointer of `q` is a DEVICE pointer.  One kernel enqueued on `hip_stream`, whatever n_segs is; asynchronous: nothing is copied
 * back and nothing synchronises.  MCQ_EINVAL before any launch, each with a message of its own: a NULL block, a mode other than
 * full_3d, N outside 2 .. 32 (33 .. 64 named as this build's limit), n_queens outside 2 .. N^3 - 1 (0 = N^2), n_chains outside
 * 1 .. 2^31 - 1, a negative n_segs or first_seg, seg_steps outside 1 .. 2^31, (first_seg + n_segs) seg_steps >= 2^50, table_len
 * outside 1 .. MCQ_MAX_NFOLD3D_TABLE, clock_ln2 outside 0 .. 2^24, a NULL seeds, state_in, state_out or clock_table, a NULL table with
 * n_segs > 0, a best_state that is state_in or state_out, hist_stride below n_segs + 1 when energy_hist is given, and any (N, Q)
 * whose chain exceeds MCQ_MAX_NFOLD3D_LDS (the message names N, Q and the bytes).  The entries of the tables, of need_in and of
 * events_in cannot be looked at here: they are the caller's. */
int mcq_nfold3d_device(const mcq_nfold3d* q, void* hip_stream);
/* The same rule in plain host code over HOST buffers, for every shape (no LDS here), otherwise the same refusals; needs no GPU.  It
 * also reads the tables and refuses a weight above 2^24, a clock_table entry above 2^26, a need_in entry >= 2^58 and a negative
 * events_in entry.  It follows the definition -- every (q, t) pair behind every event -- and is equal to the kernel bit for bit on
 * every output. */
int mcq_nfold3d_host(const mcq_nfold3d* q);

/*
 * Extremal optimisation of board placements (Boettcher and Percus, tau-EO): every iteration ranks the columns by their local
 * badness, draws a rank from a table and moves that column UNCONDITIONALLY (csrc/mcq_eo.hip) -- NOT a mode of the reference; never a
 * default, like everything above that is labelled so.  Every search above chooses a move by the energy change it causes and the
 * samplers choose by a temperature; this block has no temperature, no memory and no acceptance test.  Boards only.  The rule is
 * integer-exact:
 *   1. SETUP.  Every input byte is clamped to N - 1 first; a(c, k) and E are those of the mcq_quench rule, items 1 - 2.
 *      lambda(c) = a(c, h(c)) <= 4 (N - 1) is the local badness of column c.  No local search is applied to the input; energy_in
 *      is its recount.
 *   2. CHAIN STATE: the placement, the run's best energy B and the iteration index; nothing else.  A call runs the iterations
 *      t = 0 .. n_iters - 1; iteration t has the GLOBAL index g = first_iter + t.  B = min(best_floor[r], energy_in), or energy_in
 *      without best_floor.
 *   3. RANDOM WORDS.  Iteration g draws one block (x0, x1, x2, x3) =
 *        philox4x32-10(counter = (low 32 bits of g, high bits of g, 0, 0), key = (seeds[r], 13))
 *      (key words 0 - 12 are taken by the sweep, the two heat baths, the two tempered sweeps, mcq_hop, mcq_hop3d, mcq_tabu,
 *      mcq_tabu3d, mcq_relink, mcq_relink3d, mcq_nfold and mcq_nfold3d; this block's is 13).  o = floor(x1 N^2 / 2^32) is the tie
 *      offset of the columns and oh = floor(x2 N / 2^32) that of the heights.
 *   4. RANK.  rank_cdf is uint32[n_ranks], ONE table for all chains, 0 <= n_ranks <= N^2 - 1.  j = #{ i < n_ranks :
 *      rank_cdf[i] <= x0 }, so 0 <= j <= n_ranks.  The count is defined for any table; a table that does not decrease makes it the
 *      draw from a cumulative distribution over the ranks 0 .. n_ranks.  n_ranks = 0 gives j = 0 in every iteration.
 *   5. COLUMN.  All N^2 columns are ordered by (-lambda(c), rho(c)) ascending, rho(c) = (c - o) mod N^2: the worst first, equal
 *      lambda broken by a random rotation, so that no column order is favoured.  The iteration moves the column c at position j.  A
 *      column with lambda(c) = 0 may be drawn and moves like any other (n_free counts those moves).  With E = 0 the iteration
 *      moves nothing and counts in n_idle; that lasts forever.
 *   6. HEIGHT of the column c.  move = MCQ_EO_MOVE_BEST: the k != h(c) with the lexicographically smallest
 *      (a(c, k), (k - oh) mod N).  move = MCQ_EO_MOVE_RANDOM: k' = floor(x3 (N - 1) / 2^32) and k = k' + [k' >= h(c)].
 *      delta = a(c, k) - lambda(c).  The move is always taken: h(c) = k and E += delta.
 *   7. BEST, COUNTERS, OUTPUTS as in the mcq_tabu rule, items 5 - 6.  A move with E + delta < B sets B, best_iter = t + 1 and the
 *      best placement; best_iter is relative to the call, 0 means the input or an earlier call.  Counters, all int64: n_moves;
 *      n_uphill, the moves with delta > 0; n_flat, those with delta = 0; n_free, those of a column with lambda = 0; n_idle.
 *      energy_hist[r][0 .. n_iters] holds energy_in, then E after each iteration.  energy_out = E and state_out are those behind the
 *      last iteration.  best_energy = B.  best_state is the best placement of THIS call: when no move of the call went below B it is
 *      the (clamped) input placement, and best_energy = B <= energy_in says whether that placement has it.
 * Bounds: first_iter + n_iters < 2^63; move is MCQ_EO_MOVE_BEST or MCQ_EO_MOVE_RANDOM.
 * Consequences:
 *   (a) n_iters = 0 is the recount: state_out and best_state are the clamped input, energy_out = energy_in, best_energy = B, every
 *       counter 0.
 *   (b) a run cut into calls is the unbroken run on every output, when each call is fed state_out as state_in, best_energy as
 *       best_floor and first_iter carried over -- there is nothing else to carry; the pieces combine as under mcq_tabu (b).
 *   (c) state_out may be state_in; best_state may be neither state_in nor state_out.
 *   (d) with n_ranks = 0 and move = MCQ_EO_MOVE_BEST nothing but the ties is random: the worst column takes its best other height.
 * N = MCQ_MIN_N .. MCQ_MAX_N_QUENCH_PAIRS on the device and in host code alike.  Chains do not interact and a call reads all of a
 * chain's inputs before it writes any of its outputs.
 *
 * mcq_eo_device keeps a chain in the LDS of one wavefront: the table a(c, k) as bytes in rows of 4 ((NP / 4) | 1) bytes, the
 * heights, the best placement and NP^2 dwords for rank_cdf, NP = N rounded up to 4, 8, 12, 16, 24 or 32:
 *   bytes = NP^2 (4 ((NP / 4) | 1) + 6),  43 008 at NP = 32 (three chains per compute unit), <= MCQ_MAX_EO_LDS.
 */
#define MCQ_EO_MOVE_BEST 0
#define MCQ_EO_MOVE_RANDOM 1
#define MCQ_MAX_EO_LDS (64 * 1024) /* bytes of LDS a workgroup of mcq_eo_device may take */
typedef struct mcq_eo {
    int32_t N;              /* MCQ_MIN_N .. MCQ_MAX_N_QUENCH_PAIRS */
    int32_t mode;           /* MCQ_MODE_BOARD; anything else is MCQ_EINVAL */
    int64_t n_chains;       /* 1 .. 2^31 - 1 */
    int64_t n_iters;        /* >= 0; 0 = the recount */
    int64_t first_iter;     /* >= 0: the global index of the call's first iteration; first_iter + n_iters < 2^63 */
    int32_t move;           /* MCQ_EO_MOVE_BEST or MCQ_EO_MOVE_RANDOM */
    int32_t n_ranks;        /* 0 .. N^2 - 1: the entries of rank_cdf */
    const uint32_t* seeds;  /* [n_chains] */
    const uint32_t* rank_cdf; /* [n_ranks], one table for all chains; may be NULL when n_ranks = 0 */
    const uint8_t* state_in; /* [n_chains][N*N], final_state layout */
    uint8_t* state_out;     /* [n_chains][N*N]; may be state_in */
    const int32_t* best_floor; /* optional [n_chains]: the best energy of the calls before */
    int32_t* energy_in;     /* optional [n_chains]: E of the (clamped) input, recounted */
    int32_t* energy_out;    /* optional [n_chains]: E of the output */
    int32_t* best_energy;   /* optional [n_chains]: B */
    int64_t* best_iter;     /* optional [n_chains]: 0 = no move of the call went below B, t + 1 = behind iteration t of the call */
    uint8_t* best_state;    /* optional [n_chains][N*N]; neither state_in nor state_out */
    int64_t* n_moves;       /* optional [n_chains] */
    int64_t* n_uphill;      /* optional [n_chains]: moves with delta > 0 */
    int64_t* n_flat;        /* optional [n_chains]: moves with delta = 0 */
    int64_t* n_free;        /* optional [n_chains]: moves of a column with lambda = 0 */
    int64_t* n_idle;        /* optional [n_chains]: iterations at E = 0, which move nothing */
    int32_t* energy_hist;   /* optional [n_chains][hist_stride]: entries 0 .. n_iters */
    int64_t hist_stride;    /* >= n_iters + 1 when energy_hist is given; not read otherwise */
} mcq_eo;

/* the message of the last error of the calling thread from the two mcq_eo_* calls below (they do not set mcq_last_error()) */
const char* mcq_eo_last_error(void);
/* Every pointer of `q` is a DEVICE pointer.  One kernel enqueued on `hip_stream`, whatever n_iters is; asynchronous: nothing is
 * copied back and nothing synchronises.  MCQ_EINVAL before any launch, each with a message of its own: a NULL block, mode other than
 * board, N out of range, n_chains outside 1 .. 2^31 - 1, a negative n_iters or first_iter, first_iter + n_iters >= 2^63, a move
 * other than the two above, n_ranks outside 0 .. N^2 - 1, a NULL rank_cdf with n_ranks > 0, a NULL seeds, state_in or state_out,
 * hist_stride below n_iters + 1 when energy_hist is given, a best_state that is state_in or state_out, and a chain above
 * MCQ_MAX_EO_LDS (no N in range is).  The entries of rank_cdf cannot be looked at here: they are the caller's, and the count of
 * item 4 is defined for any of them. */
int mcq_eo_device(const mcq_eo* q, void* hip_stream);
/* The same rule in plain host code over HOST buffers -- an explicit stable sort of the columns in every iteration --, same refusals;
 * needs no GPU.  It also reads rank_cdf and refuses a table that decreases.  Equal to the kernel bit for bit on every output. */
int mcq_eo_host(const mcq_eo* q);

/*
 * Extremal optimisation of full_3d placements: every iteration ranks the QUEENS by their local badness, draws a rank from a table and
 * moves that queen UNCONDITIONALLY to a free cell of the cube (csrc/mcq_eo3d.hip) -- NOT a mode of the reference; never a default, like
 * everything above that is labelled so.  mcq_eo above keeps refusing full_3d: a queen here has N^3 targets and no column of its own,
 * and this block has its own entry points.  The rule is integer-exact:
 *   1. SETUP.  The placement (Q triples of bytes, 3 Q bytes per chain), the clamping to N - 1, REPEATED, a(q, t) and E are those of
 *      the mcq_quench3d rule, items 1 - 2, exactly as mcq_tabu3d item 1 takes them.  N = 2 .. MCQ_MAX_N_QUENCH3D and
 *      2 <= Q <= N^3 - 1 (n_queens = 0 means N^2).  C = N^3; a cell is FREE when it holds no queen, so there are F = C - Q >= 1 free
 *      cells.  lambda(q) = a(q, pos(q)) <= 13 (N - 1) is the local badness of queen q.  No local search is applied to the input;
 *      energy_in is its recount.
 *   2. CHAIN STATE: the placement, the run's best energy B and the iteration index; nothing else.  A call runs the iterations
 *      t = 0 .. n_iters - 1; iteration t has the GLOBAL index g = first_iter + t.  B = min(best_floor[r], energy_in), or energy_in
 *      without best_floor.
 *   3. RANDOM WORDS.  Iteration g draws one block (x0, x1, x2, x3) =
 *        philox4x32-10(counter = (low 32 bits of g, high bits of g, 0, 0), key = (seeds[r], 14))
 *      (key words 0 - 13 are taken by the sweep, the two heat baths, the two tempered sweeps, mcq_hop, mcq_hop3d, mcq_tabu,
 *      mcq_tabu3d, mcq_relink, mcq_relink3d, mcq_nfold, mcq_nfold3d and mcq_eo; this block's is 14).  x0 draws the rank;
 *      o_q = floor(x1 Q / 2^32) and o_t = floor(x2 C / 2^32) are the tie offsets of the queens and of the cells; x3 draws the random
 *      target.
 *   4. RANK.  rank_cdf is uint32[n_ranks], ONE table for all chains, 0 <= n_ranks <= Q - 1.  j = #{ i < n_ranks :
 *      rank_cdf[i] <= x0 }, so 0 <= j <= n_ranks.  The count is defined for any table; a table that does not decrease makes it the
 *      draw from a cumulative distribution over the ranks 0 .. n_ranks.  n_ranks = 0 gives j = 0 in every iteration.
 *   5. QUEEN.  All Q queens are ordered by (-lambda(q), rho_q) ascending, rho_q = (q - o_q) mod Q: the worst first, equal lambda
 *      broken by a random rotation, so that no queen order is favoured.  The iteration moves the queen q at position j.  A queen with
 *      lambda(q) = 0 may be drawn and moves like any other (n_free counts those moves).  With E = 0 the iteration moves nothing and
 *      counts in n_idle; that lasts forever.
 *   6. TARGET of the queen q at p = pos(q).  move = MCQ_EO3D_MOVE_BEST: the free cell t with the lexicographically smallest
 *      (a(q, t), rho_t), rho_t = (t - o_t) mod C, t the cell index i N^2 + j N + k.  move = MCQ_EO3D_MOVE_RANDOM:
 *      m = floor(x3 F / 2^32), and t is the free cell that has exactly m free cells of smaller index: uniform over the free cells.
 *      p holds a queen, so it is never a target.  delta = a(q, t) - lambda(q).  The move is always taken: pos(q) = t and E += delta.
 *   7. BEST, COUNTERS, OUTPUTS as in the mcq_eo rule, item 7: a move with E + delta < B sets B, best_iter = t + 1 and the best
 *      placement; best_iter is relative to the call, 0 means the input or an earlier call.  Counters, all int64: n_moves; n_uphill,
 *      the moves with delta > 0; n_flat, those with delta = 0; n_free, those of a queen with lambda = 0; n_idle.
 *      energy_hist[r][0 .. n_iters] holds energy_in, then E after each iteration.  energy_out = E and state_out are those behind the
 *      last iteration.  best_energy = B.  best_state is the best placement of THIS call: when no move of the call went below B it is
 *      the (clamped) input placement.  A REPEATED input (two queens in one cell after clamping) sets bit 0 of flags
 *      (MCQ_EO3D_REPEATED) and is handed back unmoved: state_out and best_state are the clamped input, energy_in = energy_out =
 *      best_energy = the recount (a shared cell counts as an attacking pair; best_floor is not looked at), every counter and best_iter
 *      are 0, and energy_hist[0 .. n_iters] all hold the recount.  No output of the rule is such a placement.
 * Bounds: first_iter + n_iters < 2^63; move is MCQ_EO3D_MOVE_BEST or MCQ_EO3D_MOVE_RANDOM.
 * Consequences:
 *   (a) n_iters = 0 is the recount: state_out and best_state are the clamped input, energy_out = energy_in, best_energy = B, every
 *       counter 0.
 *   (b) a run cut into calls is the unbroken run on every output, when each call is fed state_out as state_in, best_energy as
 *       best_floor and first_iter carried over -- there is nothing else to carry; the pieces combine as under mcq_tabu (b).
 *   (c) state_out may be state_in; best_state may be neither state_in nor state_out.
 *   (d) with n_ranks = 0 and move = MCQ_EO3D_MOVE_BEST nothing but the ties is random: the worst queen takes its best free cell.
 * Chains do not interact and a call reads all of a chain's inputs before it writes any of its outputs.
 *
 * mcq_eo3d_device keeps a chain in the LDS of one workgroup: 480 dwords (two of 32 for the reductions and 416 bins of lambda), the
 * field (one byte per cell to N = 19, 16 bits beyond), the occupancy bitmap and the queens (16 bits each), each array rounded up to a
 * dword; rank_cdf stays in global memory:
 *   bytes = 4 (480 + ceil(N^3 / (4 or 2)) + ceil(N^3 / 32) + ceil(Q / 2)) <= MCQ_MAX_EO3D_LDS.
 * Every shape fits: 137 088 bytes at N = 32 with Q = N^3 - 1.
 */
#define MCQ_EO3D_MOVE_BEST 0
#define MCQ_EO3D_MOVE_RANDOM 1
#define MCQ_MAX_EO3D_LDS (160 * 1024) /* bytes of LDS a workgroup of mcq_eo3d_device may take */
#define MCQ_EO3D_REPEATED 1 /* flags bit 0: two queens of the (clamped) input hold the same cell; nothing was moved */
typedef struct mcq_eo3d {
    int32_t N;              /* MCQ_MIN_N .. MCQ_MAX_N_QUENCH3D */
    int32_t n_queens;       /* Q: 2 .. N^3 - 1; 0 = N^2 */
    int64_t n_chains;       /* 1 .. 2^31 - 1 */
    int64_t n_iters;        /* >= 0; 0 = the recount */
    int64_t first_iter;     /* >= 0: the global index of the call's first iteration; first_iter + n_iters < 2^63 */
    int32_t move;           /* MCQ_EO3D_MOVE_BEST or MCQ_EO3D_MOVE_RANDOM */
    int32_t n_ranks;        /* 0 .. Q - 1: the entries of rank_cdf */
    const uint32_t* seeds;  /* [n_chains] */
    const uint32_t* rank_cdf; /* [n_ranks], one table for all chains; may be NULL when n_ranks = 0 */
    const uint8_t* state_in; /* [n_chains][Q][3], final_state layout of full_3d */
    uint8_t* state_out;     /* [n_chains][Q][3]; may be state_in */
    const int32_t* best_floor; /* optional [n_chains]: the best energy of the calls before */
    int32_t* energy_in;     /* optional [n_chains]: E of the (clamped) input, recounted */
    int32_t* energy_out;    /* optional [n_chains]: E of the output */
    int32_t* best_energy;   /* optional [n_chains]: B */
    int64_t* best_iter;     /* optional [n_chains]: 0 = no move of the call went below B, t + 1 = behind iteration t of the call */
    uint8_t* best_state;    /* optional [n_chains][Q][3]; neither state_in nor state_out */
    int64_t* n_moves;       /* optional [n_chains] */
    int64_t* n_uphill;      /* optional [n_chains]: moves with delta > 0 */
    int64_t* n_flat;        /* optional [n_chains]: moves with delta = 0 */
    int64_t* n_free;        /* optional [n_chains]: moves of a queen with lambda = 0 */
    int64_t* n_idle;        /* optional [n_chains]: iterations at E = 0, which move nothing */
    int32_t* energy_hist;   /* optional [n_chains][hist_stride]: entries 0 .. n_iters */
    int64_t hist_stride;    /* >= n_iters + 1 when energy_hist is given; not read otherwise */
    int32_t* flags;         /* optional [n_chains]: MCQ_EO3D_* */
} mcq_eo3d;

/* the message of the last error of the calling thread from the two mcq_eo3d_* calls below (they do not set mcq_last_error()) */
const char* mcq_eo3d_last_error(void);
/* Every pointer of `q` is a DEVICE pointer.  One kernel enqueued on `hip_stream`, whatever n_iters is; asynchronous: nothing is
 * copied back and nothing synchronises.  MCQ_EINVAL before any launch, each with a message of its own: a NULL block, N outside
 * 2 .. 32 (33 .. 64 named as this build's limit), n_queens outside 2 .. N^3 - 1 (0 = N^2), n_chains outside 1 .. 2^31 - 1, a negative
 * n_iters or first_iter, first_iter + n_iters >= 2^63, a move other than the two above, n_ranks outside 0 .. Q - 1, a NULL rank_cdf
 * with n_ranks > 0, a NULL seeds, state_in or state_out, hist_stride below n_iters + 1 when energy_hist is given, a best_state that
 * is state_in or state_out, and a chain above MCQ_MAX_EO3D_LDS (no shape in range is).  The entries of rank_cdf cannot be looked at
 * here: they are the caller's, and the count of item 4 is defined for any of them. */
int mcq_eo3d_device(const mcq_eo3d* q, void* hip_stream);
/* The same rule in plain host code over HOST buffers -- an explicit stable sort of the queens in every iteration and a loop over the
 * cells for the target --, same refusals; needs no GPU.  It also reads rank_cdf and refuses a table that decreases.  Equal to the
 * kernel bit for bit on every output. */
int mcq_eo3d_host(const mcq_eo3d* q);

/* ---- exported by libmcq_oracle.so (tests / smoke / cpu_baseline only) --------------------- */

/* CPU restatement of the reference; host buffers; n_threads <= 1 runs chains in the calling thread. */
int mcq_oracle_run(const mcq_params* p, const uint32_t* seeds, const mcq_outputs* out, int n_threads);
/* the same chains with O(1) dE from per-line occupancy counters: the "best CPU" baseline of bench.py; equals mcq_oracle_run */
int mcq_oracle_run_fast(const mcq_params* p, const uint32_t* seeds, const mcq_outputs* out, int n_threads);
/* one Philox-4x32-10 block: ctr[4], key[2] -> out[4] (known-answer tests) */
int mcq_oracle_philox_block(const uint32_t* ctr, const uint32_t* key, uint32_t* out);
const char* mcq_oracle_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* MCQ_H */
