// mcq_hop3d.hip -- basin hopping of full_3d placements: kick a few queens of a minimum to free cells, descend again, keep the new minimum
// when it is no worse and go back otherwise (include/mcq.h: mcq_hop3d, where the rule is stated).  The local search is the descent of
// csrc/mcq_quench3d.hip, restated here so that file stays as it is; what this file adds is the loop around it, as one launch.
//
//   kernel  one chain per workgroup of W lanes, all in LDS, laid out as in the quench (csrc/mcq_field.h): red, 32 dwords, then the field,
//           occ and the queens, and behind them prev, Q more packed cells: the placement from before the kick, written behind the first
//           descent and behind every accepted hop.  The field is built ONCE per launch.
//           KICK: the Philox block and the draw (n, t) are computed by every lane from uniform values; the draw is refused or taken on
//           one bit of occ, read behind a barrier.  A draw that moves queen n from p to t changes E by S(t) - [p attacks t] - (S(p) - 1),
//           read before anything is written; then the -1 on p's lines and the +1 on t's go out together: the field is additive.
//           DESCENT: the pass loop of the quench kernel.
//           RESTORE: on a rejected hop the queens with queens[q] != prev[q] return.  Their bits of occ are cleared, and behind a
//           barrier the bits of their old cells are set (a cell one queen left may be the cell another returns to); their -1 and +1
//           on the field go out as one loop over (queen, slot) pairs, like the first build.  A dword of the field may carry from one
//           entry into the next while both signs are under way: the adds are exact modulo 2^32 and nothing reads before the barrier.
//           Every branch on the chain's data (draw taken, queen skipped, hop accepted, descent ended) is taken on values every lane
//           read from LDS behind a barrier or computed alike, so every barrier is reached by all lanes.  best_state goes to global
//           memory behind the first descent and when a hop improves; state_out at the end; energy_hist by one lane.
//   host    mcq_hop3d_host: the same rule on HostField with plain loops.
//
// Built for gfx950 only, with csrc/mcq_hip.hip:  hipcc --offload-arch=gfx950 -O3 -ffp-contract=off
#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/mcq.h"
#include "mcq_field.h"
#include "mcq_post.h"

namespace {

using namespace mcq_field;
using mcq_post::fail;
using mcq_post::philox_block;
using mcq_post::queens_of;

thread_local char g_hop3d_err[256] = "";

constexpr uint32_t HOP3D_KEY_WORD = 6u;  // key word 1 of the chain's Philox stream: 0 - 5 are the sweep's, the heat baths', the tempered sweeps' and mcq_hop's

struct Hop3dArgs {
    const uint32_t* seeds;
    const uint8_t* state_in;
    uint8_t* state_out;
    int32_t* energy_in;
    int32_t* energy_start;
    int32_t* energy_out;
    int32_t* best_energy;
    int64_t* best_hop;
    uint8_t* best_state;
    int64_t* n_accepted;
    int64_t* n_improved;
    int64_t* n_moves;
    int64_t* n_passes;
    int64_t* n_kicked;
    int32_t* energy_hist;
    int32_t* flags;
    long long hist_stride;
    long long n_hops;
    long long first_hop;
    int kick;
    int slack;
    int N;
    int Q;
};

// the per-chain figures, by one lane or by the host: `a` is the kernel's argument struct or the parameter block
template <class A>
__host__ __device__ __forceinline__ void store_hop3d_figures(const A& a, long long ch, int e_in, int e_start, int E, int best, long long best_hop,
                                                             long long accepted, long long improved, long long moves, long long passes,
                                                             long long kicked, int flags) {
    if (a.energy_in) a.energy_in[ch] = e_in;
    if (a.energy_start) a.energy_start[ch] = e_start;
    if (a.energy_out) a.energy_out[ch] = E;
    if (a.best_energy) a.best_energy[ch] = best;
    if (a.best_hop) a.best_hop[ch] = best_hop;
    if (a.n_accepted) a.n_accepted[ch] = accepted;
    if (a.n_improved) a.n_improved[ch] = improved;
    if (a.n_moves) a.n_moves[ch] = moves;
    if (a.n_passes) a.n_passes[ch] = passes;
    if (a.n_kicked) a.n_kicked[ch] = kicked;
    if (a.flags) a.flags[ch] = flags;
}

// draw d of the kick of hop g: words 2 (g m + d) and 2 (g m + d) + 1 of the chain's stream, as (queen n, cell t).  `lo` and `hi` hold the
// two halves of the block of the draw before (a block serves two draws) as 64-bit words -- scalars, not an array, so that picking a half
// is a select and nothing goes to scratch --; `fresh` says that they do not.
__host__ __device__ __forceinline__ void kick_draw(uint32_t seed, unsigned long long g, int m, int d, int Q, int C, bool fresh, unsigned long long& lo,
                                                   unsigned long long& hi, int& n, int& t) {
    const unsigned long long w = 2ull * (g * (unsigned long long)m + (unsigned long long)d);
    if (fresh || (w & 3) == 0) {
        uint32_t r[4];
        philox_block((uint32_t)(w >> 2), (uint32_t)(w >> 34), seed, HOP3D_KEY_WORD, r);
        lo = (unsigned long long)r[0] | ((unsigned long long)r[1] << 32);
        hi = (unsigned long long)r[2] | ((unsigned long long)r[3] << 32);
    }
    const unsigned long long x = (w & 2) != 0 ? hi : lo;
    n = (int)(((x & 0xFFFFFFFFull) * (unsigned)Q) >> 32);
    t = (int)(((x >> 32) * (unsigned)C) >> 32);
}

template <int W, int BITS, int STEPS>
__global__ __launch_bounds__(W) void mcq_hop3d_kernel(Hop3dArgs a) {
    extern __shared__ uint32_t lds[];
    constexpr int CPD = 32 / BITS, SLOTS = 13 * STEPS;
    const int N = a.N, Q = a.Q, N2 = N * N, C = N2 * N;
    uint32_t* red = lds;
    const Chain chain = carve<BITS>(lds + 32, C);
    uint32_t* const field = chain.field;
    uint32_t* const occ = chain.occ;
    uint16_t* const queens = chain.queens;
    uint16_t* const prev = queens + 2 * ((Q + 1) / 2);  // behind the queens, on a dword
    const int fw = chain.fw, bw = chain.bw;
    const int tid = threadIdx.x;
    const long long ch = blockIdx.x;
    const uint32_t seed = a.seeds[ch];
    const uint8_t* in = a.state_in + ch * 3 * Q;
    uint8_t* out = a.state_out + ch * 3 * Q;
    uint8_t* bs = a.best_state ? a.best_state + ch * 3 * Q : nullptr;
    int32_t* hist = a.energy_hist ? a.energy_hist + ch * a.hist_stride : nullptr;

    for (int w = tid; w < fw + bw; w += W) field[w] = 0;  // (field and occ are adjacent)
    __syncthreads();
    if (tid == 0) set_pad_bits(occ, bw, C);
    __syncthreads();
    int rep = 0;
    for (int q = tid; q < Q; q += W) rep |= load_queen(queens, occ, in, N, q);
    __syncthreads();  // queens and occ are complete, every byte of state_in is read
    const bool repeated = block_sum<W>(rep, red) != 0;  // (through red, not __syncthreads_or: that keeps static LDS, which the byte bound does not count)

    if (repeated) {  // rule item 7: recounted pair by pair, handed back unmoved
        int twoE = 0;
        for (int q = tid; q < Q; q += W) {
            const int p = queens[q];
            int n = 0;
            for (int o = 0; o < Q; o++) n += attacks(p, queens[o]);
            twoE += n - 1;  // itself
            store_queen(out, q, p);
            if (bs) store_queen(bs, q, p);
        }
        const int e = block_sum<W>(twoE, red) >> 1;
        if (hist)
            for (long long t = tid; t <= a.n_hops; t += W) hist[t] = e;
        if (tid == 0) store_hop3d_figures(a, ch, e, e, e, e, 0, 0, 0, 0, 0, 0, MCQ_HOP3D_REPEATED);
        return;
    }

    for (int x = tid; x < Q * SLOTS; x += W) put_slot<W, BITS, STEPS>(field, queens, N, x);
    __syncthreads();
    int twoE = 0;
    for (int q = tid; q < Q; q += W) twoE += attackers_at<BITS>(field, N, queens[q]);
    const int e_in = block_sum<W>(twoE, red) >> 1;

    int E = e_in, e_start = e_in, best = e_in;
    long long moves = 0, passes = 0, kicked = 0, accepted = 0, improved = 0, best_hop = 0;
    const int m = a.kick;
    // t = -1 is the descent of the input (rule item 3); t >= 0 are the hops
    for (long long t = -1; t < a.n_hops; t++) {
        const int e_prev = E;
        __syncthreads();  // the field, occ, the queens and prev are the chain's: nothing of the hop before is under way
        if (t >= 0) {     // the kick
            const unsigned long long g = (unsigned long long)(a.first_hop + t);
            unsigned long long lo = 0, hi = 0;
            for (int d = 0; d < m; d++) {
                int n, tcell;
                kick_draw(seed, g, m, d, Q, C, d == 0, lo, hi, n, tcell);
                if ((occ[tcell >> 5] >> (tcell & 31)) & 1u) continue;  // (uniform: every lane read the same bit behind a barrier)
                const int p = queens[n];
                const int pcell = cell_of(p, N);
                const int tp = packed_of(tcell, N, N2);
                E += field_at<BITS>(field, tcell) - (int)attacks(p, tp) - (field_at<BITS>(field, pcell) - 1);
                kicked++;
                __syncthreads();  // every lane has read the bit, queens[n], S(t) and S(p) before the queen moves
                put<W, BITS, STEPS>(field, N, p, -1, tid, W, SLOTS);
                put<W, BITS, STEPS>(field, N, tp, +1, tid, W, SLOTS);
                if (tid == 0) {
                    vacate(occ, pcell);
                    occupy(occ, queens, n, tp, tcell);
                }
                __syncthreads();
            }
        }

        // the descent: the pass loop of csrc/mcq_quench3d.hip
        const int e0 = E;
        int lm = 0, lp = 0;
        for (;;) {
            int moved = 0;
            for (int q = 0; q < Q; q++) {
                const int p = queens[q];
                const int pcell = cell_of(p, N);
                const int now = field_at<BITS>(field, pcell) - 1;
                if (now == 0) continue;  // (uniform: every lane read the same entries)
                __syncthreads();         // every lane has read S(p) before the queen is taken out
                put<W, BITS, STEPS>(field, N, p, -1, tid, W, SLOTS);
                if (tid == 0) vacate(occ, pcell);
                __syncthreads();
                uint32_t key = ~0u;
                for (int w = tid; w < fw; w += W) {
                    const uint32_t v = field[w];
                    const uint32_t o = occ[(w * CPD) >> 5] >> ((w * CPD) & 31);
#pragma unroll
                    for (int b = 0; b < CPD; b++)
                        if (!((o >> b) & 1u)) key = min(key, ((v >> (b * BITS)) & ((1u << BITS) - 1u)) << 16 | (uint32_t)(w * CPD + b));
                }
                key = block_min<W, true>(key, red);
                const int low = (int)(key >> 16);
                int tq = p, tcell = pcell;
                if (low < now) {
                    tcell = (int)(key & 0xffffu);
                    tq = packed_of(tcell, N, N2);
                    E += low - now;
                    moved++;
                }
                __syncthreads();  // every lane has read queens[q] and the whole field before the queen goes back
                put<W, BITS, STEPS>(field, N, tq, +1, tid, W, SLOTS);
                if (tid == 0) occupy(occ, queens, q, tq, tcell);
                __syncthreads();
            }
            lp++;
            lm += moved;
            // (lp > e0 cannot happen -- every moving pass lowers E --: it only bounds the loop should the rule ever be broken)
            if (moved == 0 || lp > e0) break;
        }
        moves += lm, passes += lp;

        bool keeps = true, improves = false;
        if (t < 0) {
            e_start = best = E;
            improves = true;  // best_state to begin with
        } else if ((long long)E <= (long long)e_prev + a.slack) {
            accepted++;
            if (E < best) best = E, best_hop = t + 1, improved++, improves = true;
        } else {  // back to the cells before the kick
            keeps = false;
            __syncthreads();
            for (int q = tid; q < Q; q += W) {
                const int cur = queens[q];
                if (cur != prev[q]) {
                    const int c = cell_of(cur, N);
                    atomicAnd(&occ[c >> 5], ~(1u << (c & 31)));
                }
            }
            __syncthreads();  // every bit of a cell that is left is cleared before a bit of a cell that is taken again is set
            for (int q = tid; q < Q; q += W) {
                const int old = prev[q];
                if (old != queens[q]) {
                    const int c = cell_of(old, N);
                    atomicOr(&occ[c >> 5], 1u << (c & 31));
                }
            }
            for (int x = tid; x < Q * SLOTS; x += W) {
                const int q = x / SLOTS, s = x - q * SLOTS;
                const int cur = queens[q], old = prev[q];
                if (cur != old) {
                    put<W, BITS, STEPS>(field, N, cur, -1, s, SLOTS, SLOTS);
                    put<W, BITS, STEPS>(field, N, old, +1, s, SLOTS, SLOTS);
                }
            }
            __syncthreads();  // every lane has compared queens with prev
            for (int q = tid; q < Q; q += W) queens[q] = prev[q];
            E = e_prev;
        }
        if (keeps) {  // the first descent and an accepted hop: the placement is the chain's
            for (int q = tid; q < Q; q += W) prev[q] = queens[q];
        }
        if (improves && bs) store_queens(bs, queens, Q, tid, W);
        if (hist && tid == 0) hist[t + 1] = E;
    }

    __syncthreads();
    store_queens(out, queens, Q, tid, W);
    if (tid == 0) store_hop3d_figures(a, ch, e_in, e_start, E, best, best_hop, accepted, improved, moves, passes, kicked, 0);
}

// what both entry points refuse
int check_hop3d(const mcq_hop3d* q) {
    if (!q) return fail(g_hop3d_err, MCQ_EINVAL, "mcq_hop3d: NULL parameter block");
    const int rc = mcq_post::check_full3d(g_hop3d_err, "hop", q->N, q->n_queens, (long long)q->n_chains);
    if (rc != MCQ_OK) return rc;
    if (q->n_hops < 0) return fail(g_hop3d_err, MCQ_EINVAL, "n_hops must be >= 0 (0 = the local search alone), got %lld", (long long)q->n_hops);
    if (q->first_hop < 0) return fail(g_hop3d_err, MCQ_EINVAL, "first_hop must be >= 0, got %lld", (long long)q->first_hop);
    if (q->slack < 0) return fail(g_hop3d_err, MCQ_EINVAL, "slack must be >= 0, got %d", (int)q->slack);
    if (q->kick < 1 || q->kick > MCQ_MAX_HOP_KICK) return fail(g_hop3d_err, MCQ_EINVAL, "kick out of range [1, %d]: %d", MCQ_MAX_HOP_KICK, (int)q->kick);
    const unsigned __int128 words = (unsigned __int128)2 * (unsigned)q->kick * ((unsigned __int128)q->first_hop + (unsigned __int128)q->n_hops);
    if (words >= ((unsigned __int128)1 << 63))
        return fail(g_hop3d_err, MCQ_EINVAL, "stream words: 2 kick (first_hop + n_hops) must stay below 2^63 (kick %d, first_hop %lld, n_hops %lld)",
                    (int)q->kick, (long long)q->first_hop, (long long)q->n_hops);
    if (!q->seeds) return fail(g_hop3d_err, MCQ_EINVAL, "seeds is required");
    if (!q->state_in) return fail(g_hop3d_err, MCQ_EINVAL, "state_in is required");
    if (!q->state_out) return fail(g_hop3d_err, MCQ_EINVAL, "state_out is required");
    if (q->energy_hist && q->hist_stride < q->n_hops + 1)
        return fail(g_hop3d_err, MCQ_EINVAL, "hist_stride must be >= n_hops + 1 = %lld, got %lld", (long long)q->n_hops + 1, (long long)q->hist_stride);
    return MCQ_OK;
}

// the bytes of LDS of a chain: red, the field, occ, the queens and prev
long long lds_bytes(int N, int Q) {
    const long long cells = (long long)N * N * N, cpd = N <= 19 ? 4 : 2;
    return 4 * (32 + (cells + cpd - 1) / cpd + (cells + 31) / 32 + 2 * (((long long)Q + 1) / 2));
}

// chains first .. last - 1 through the rule, with an int field per cell
void host_chains(const mcq_hop3d* q, long long first, long long last) {
    const int Q = queens_of(q);
    HostField f(q->N, Q);
    const std::vector<int>& S = f.S;
    std::vector<int> prev((size_t)Q);
    long long moves = 0, passes = 0;
    int E = 0;
    // L: passes of the quench rule until one moves nothing
    auto descend = [&]() {
        for (;;) {
            int moved = 0;
            for (int n = 0; n < Q; n++) {
                const int p = f.pos[(size_t)n], now = S[(size_t)p] - 1;
                if (now == 0) continue;  // no cell can hold less
                f.take_out(n);
                int t = -1;
                for (int c = 0; c < f.C; c++)
                    if (!f.occ[(size_t)c] && (t < 0 || S[(size_t)c] < S[(size_t)t])) t = c;  // strictly: the smallest cell of the minimum
                if (S[(size_t)t] < now) {
                    E += S[(size_t)t] - now;
                    moved++;
                } else {
                    t = p;
                }
                f.put_back(n, t);
            }
            passes++;
            moves += moved;
            if (moved == 0) break;
        }
    };
    for (long long ch = first; ch < last; ch++) {
        const bool repeated = f.load(q->state_in + ch * 3 * Q);
        const int e_in = f.energy();
        uint8_t* bs = q->best_state ? q->best_state + ch * 3 * Q : nullptr;
        int32_t* hist = q->energy_hist ? q->energy_hist + ch * q->hist_stride : nullptr;
        if (repeated) {
            f.store(q->state_out + ch * 3 * Q);
            if (bs) f.store(bs);
            if (hist)
                for (long long t = 0; t <= q->n_hops; t++) hist[t] = e_in;
            store_hop3d_figures(*q, ch, e_in, e_in, e_in, e_in, 0, 0, 0, 0, 0, 0, MCQ_HOP3D_REPEATED);
            continue;
        }
        moves = passes = 0;
        E = e_in;
        descend();
        const int e_start = E;
        int best = E;
        long long kicked = 0, accepted = 0, improved = 0, best_hop = 0;
        prev = f.pos;
        if (bs) f.store(bs);
        if (hist) hist[0] = E;
        const uint32_t seed = q->seeds[ch];
        for (long long t = 0; t < q->n_hops; t++) {
            const int e_prev = E;
            unsigned long long lo = 0, hi = 0;
            for (int d = 0; d < q->kick; d++) {
                int n, cell;
                kick_draw(seed, (unsigned long long)(q->first_hop + t), q->kick, d, Q, f.C, d == 0, lo, hi, n, cell);
                if (f.occ[(size_t)cell]) continue;  // the cell holds a queen: the draw moves nothing
                const int p = f.pos[(size_t)n];
                f.take_out(n);
                E += S[(size_t)cell] - S[(size_t)p];
                f.put_back(n, cell);
                kicked++;
            }
            descend();
            if ((long long)E <= (long long)e_prev + q->slack) {
                prev = f.pos;
                accepted++;
                if (E < best) {
                    best = E, best_hop = t + 1, improved++;
                    if (bs) f.store(bs);
                }
            } else {  // every queen that moved leaves, then every one of them returns
                for (int n = 0; n < Q; n++)
                    if (f.pos[(size_t)n] != prev[(size_t)n]) f.take_out(n);
                for (int n = 0; n < Q; n++)
                    if (f.pos[(size_t)n] != prev[(size_t)n]) f.put_back(n, prev[(size_t)n]);
                E = e_prev;
            }
            if (hist) hist[t + 1] = E;
        }
        f.store(q->state_out + ch * 3 * Q);
        store_hop3d_figures(*q, ch, e_in, e_start, E, best, best_hop, accepted, improved, moves, passes, kicked, 0);
    }
}

}  // namespace

extern "C" {

const char* mcq_hop3d_last_error(void) { return g_hop3d_err; }

int mcq_hop3d_host(const mcq_hop3d* q) {
    const int rc = check_hop3d(q);
    if (rc != MCQ_OK) return rc;
    mcq_post::for_chains((long long)q->n_chains, [q](long long first, long long last) { host_chains(q, first, last); });
    return MCQ_OK;
}

int mcq_hop3d_device(const mcq_hop3d* q, void* hip_stream) {
    const int rc = check_hop3d(q);
    if (rc != MCQ_OK) return rc;
    const int Q = queens_of(q);
    const long long bytes = lds_bytes(q->N, Q);
    if (bytes > MCQ_MAX_HOP3D_LDS)
        return fail(g_hop3d_err, MCQ_EINVAL, "N = %d with n_queens = %d: a chain takes %lld bytes of LDS, above the %d of a workgroup "
                    "(mcq_hop3d_device runs every Q = N^2; mcq_hop3d_host runs every shape)", (int)q->N, Q, bytes, MCQ_MAX_HOP3D_LDS);
    hipStream_t s = (hipStream_t)hip_stream;
    const Hop3dArgs a{q->seeds, q->state_in, q->state_out, q->energy_in, q->energy_start, q->energy_out, q->best_energy, q->best_hop, q->best_state,
                      q->n_accepted, q->n_improved, q->n_moves, q->n_passes, q->n_kicked, q->energy_hist, q->flags, (long long)q->hist_stride,
                      (long long)q->n_hops, (long long)q->first_hop, (int)q->kick, (int)q->slack, (int)q->N, Q};
    const hipError_t e = for_shape_of(a.N, [&](auto shape) {
        using S = decltype(shape);
        return launch<S>(mcq_hop3d_kernel<S::W, S::BITS, S::STEPS>, a, a.N, a.Q, 32 + (a.Q + 1) / 2, (long long)q->n_chains, s);
    });
    if (e != hipSuccess) return fail(g_hop3d_err, MCQ_EDEVICE, "mcq_hop3d_device: %s", hipGetErrorString(e));
    return MCQ_OK;
}

}  // extern "C"
