// mcq_eo3d.hip -- extremal optimisation of full_3d placements (tau-EO): every iteration ranks the Q queens by their local badness
// lambda(q) = a(q, pos(q)), draws a rank from one table and moves the queen at that rank unconditionally to a free cell of the cube
// (include/mcq.h: mcq_eo3d, where the rule is stated).  The field, its update and the start of a chain are those of csrc/mcq_field.h, as
// in csrc/mcq_tabu3d.hip; what this file adds is the rank search over lambda and the draw of a free cell, as one launch.
//
//   kernel  one chain per workgroup of W lanes, all in LDS: red, 32 dwords; aux, 32 dwords (a dword per wavefront and one for the
//           winner of a search); 416 bins of a histogram of lambda; then the field S of the WHOLE placement, occ and the queens
//           (csrc/mcq_field.h).  The field is built ONCE per launch.  rank_cdf stays in global memory: it is one table for all chains
//           and may hold 32 766 dwords.
//           ITERATION: (1) the Philox block, from values that are uniform over the workgroup.  (2) j, a count over rank_cdf, every lane
//           taking entries W apart, then block_sum.  (3) lambda(q) = S(pos q) - 1 of every queen into the bins, LDS atomics.  (4) every
//           wavefront scans the bins from the worst down, 64 lanes with ceil(bins / 64) bins each and a shuffle scan over the lanes: the
//           value class v of position j, and `above` = #{lambda > v}.  (5) THE RANK SEARCH sorts nothing.  The ordinal of the queen
//           inside the class in the order of rho_q is m = j - above; with n_lo the members of the class below o_q, that is the ordinal
//           (m + n_lo) mod |class| in the order of q.  Wavefront w owns the queens 64 L w .. 64 L (w + 1) - 1, L = ceil(Q / W), in
//           rounds of 64: ballots give its members and those below o_q, a dword per wavefront in aux gives every lane the members in
//           front of its wavefront, and the one wavefront whose range holds the ordinal walks its rounds again and names q (mbcnt
//           inside a round).  (6) the queen is taken out with put(-1), so that S(t) IS a(q, t) at every cell.  BEST: one pass over the
//           field and occupancy dwords, block_min of S << 15 | rho_t over the free cells (the queen's own cell still holds its bit in
//           occ: never a target).  RANDOM: occ has at most W dwords in every shape, so each lane counts the free cells of ONE dword
//           (the pad bits are set: not free), a scan over the workgroup, and the lane whose dword holds the m-th free cell picks the
//           bit.  (7) put(+1) at t, occupy, E, the counters, and best_state to global memory when B falls.
//           Every branch around a barrier (an iteration at E = 0, the move kind, B falling, the REPEATED chain) is taken on values that
//           every lane computed alike from the arguments or read from LDS behind a barrier, so every barrier is reached by all lanes.
//           The branches taken by one wavefront or one lane alone (the scan's walk, the walk of the owning wavefront, the lane that
//           picks the bit) hold no barrier.
//   host    mcq_eo3d_host: the same rule on HostField with plain loops, following the definition: an explicit std::stable_sort of the
//           queens by (-lambda, rho_q) in every iteration and a loop over the cells for the target, with the queen taken out.  It
//           shares nothing with the kernel's rank search.
//
// Built for gfx950 only, with csrc/mcq_hip.hip:  hipcc --offload-arch=gfx950 -O3 -ffp-contract=off
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <vector>

#include "../../include/mcq.h"
#include "mcq_field.h"
#include "mcq_post.h"

namespace {

using namespace mcq_field;
using mcq_post::fail;
using mcq_post::philox_block;
using mcq_post::queens_of;

thread_local char g_eo3d_err[256] = "";

constexpr uint32_t EO3D_KEY_WORD = 14u;  // key word 1 of the chain's Philox stream: 0 - 13 are taken (include/mcq.h)
constexpr int RHO_BITS = 15;             // rho_t < N^3 <= 32^3
constexpr uint32_t RHO_MASK = (1u << RHO_BITS) - 1u;
constexpr uint32_t KEY_NONE = 0xFFFFFFFFu;  // a cell key S << 15 | rho_t stays below 2^24 (S <= 13 (N - 1) + 1 = 404 < 2^9)
constexpr int AUX = 32;                     // dwords of aux: one per wavefront (16 at most), and AUX_PICK
constexpr int AUX_PICK = 16;                // the queen, then the cell, that a search found
constexpr int BINS = 416;                   // dwords of the histogram: lambda <= 13 (N - 1) <= 403
constexpr int EXTRA = 32 + AUX + BINS;      // dwords in front of the field: 480
static_assert(13 * (MCQ_MAX_N_QUENCH3D - 1) + 1 <= BINS, "a bin per value of lambda");

struct Eo3dArgs {
    const uint32_t* seeds;
    const uint32_t* rank_cdf;
    const uint8_t* state_in;
    uint8_t* state_out;
    const int32_t* best_floor;
    int32_t* energy_in;
    int32_t* energy_out;
    int32_t* best_energy;
    int64_t* best_iter;
    uint8_t* best_state;
    int64_t* n_moves;
    int64_t* n_uphill;
    int64_t* n_flat;
    int64_t* n_free;
    int64_t* n_idle;
    int32_t* energy_hist;
    int32_t* flags;
    long long hist_stride;
    long long n_iters;
    long long first_iter;
    int move;
    int n_ranks;
    int N;
    int Q;
};

// the per-chain figures, by one lane or by the host: `a` is the kernel's argument struct or the parameter block
template <class A>
__host__ __device__ __forceinline__ void store_eo3d_figures(const A& a, long long ch, int e_in, int E, int B, long long best_iter, long long moves,
                                                            long long uphill, long long flat, long long free_moves, long long idle, int flags) {
    if (a.energy_in) a.energy_in[ch] = e_in;
    if (a.energy_out) a.energy_out[ch] = E;
    if (a.best_energy) a.best_energy[ch] = B;
    if (a.best_iter) a.best_iter[ch] = best_iter;
    if (a.n_moves) a.n_moves[ch] = moves;
    if (a.n_uphill) a.n_uphill[ch] = uphill;
    if (a.n_flat) a.n_flat[ch] = flat;
    if (a.n_free) a.n_free[ch] = free_moves;
    if (a.n_idle) a.n_idle[ch] = idle;
    if (a.flags) a.flags[ch] = flags;
}

// the words of iteration g: x0 for the rank, the tie offsets o_q of the queens and o_t of the cells, and x3 for a random target
__host__ __device__ __forceinline__ void eo3d_draw(uint32_t seed, unsigned long long g, int Q, int C, uint32_t& x0, int& oq, int& ot, uint32_t& x3) {
    uint32_t r[4];
    philox_block((uint32_t)g, (uint32_t)(g >> 32), seed, EO3D_KEY_WORD, r);
    x0 = r[0];
    oq = (int)(((unsigned long long)r[1] * (unsigned)Q) >> 32);
    ot = (int)(((unsigned long long)r[2] * (unsigned)C) >> 32);
    x3 = r[3];
}

// rule item 6, the random move: the ordinal of the target among the F free cells
__host__ __device__ __forceinline__ int eo3d_ordinal(uint32_t x3, int F) { return (int)(((unsigned long long)x3 * (unsigned)F) >> 32); }

// the lanes of the wavefront below this one whose bit is set in b
__device__ __forceinline__ int ballot_prefix(unsigned long long b) {
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
}

// the sum of v over this lane and the lanes of its wavefront below it
__device__ __forceinline__ int wave_scan(int v) {
    const int lane = threadIdx.x & 63;
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(v, o, 64);
        v += lane >= o ? t : 0;
    }
    return v;
}

template <int W, int BITS, int STEPS>
__global__ __launch_bounds__(W) void mcq_eo3d_kernel(Eo3dArgs a) {
    extern __shared__ uint32_t lds[];
    constexpr int CPD = 32 / BITS, SLOTS = 13 * STEPS, WAVES = W / 64;
    const int N = a.N, Q = a.Q, N2 = N * N, C = N2 * N;
    uint32_t* const red = lds;
    uint32_t* const aux = lds + 32;
    uint32_t* const bins = lds + 32 + AUX;
    const Chain chain = carve<BITS>(lds + EXTRA, C);
    uint32_t* const field = chain.field;
    uint32_t* const occ = chain.occ;
    uint16_t* const queens = chain.queens;
    const int fw = chain.fw, bw = chain.bw;  // bw <= W in every shape: 54 of 64 at N = 12, 215 of 256 at N = 19, 1024 of 1024 at N = 32
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long ch = blockIdx.x;
    const uint32_t seed = a.seeds[ch];
    const uint8_t* in = a.state_in + ch * 3 * Q;
    uint8_t* out = a.state_out + ch * 3 * Q;
    uint8_t* bs = a.best_state ? a.best_state + ch * 3 * Q : nullptr;
    int32_t* hist = a.energy_hist ? a.energy_hist + ch * a.hist_stride : nullptr;
    const int n_bins = 13 * (N - 1) + 1, per_lane = (n_bins + 63) >> 6;  // the bins 0 .. 13 (N - 1), and those of a lane in the scan
    const int rounds = (Q + W - 1) / W;                                    // of a wavefront over its 64 `rounds` queens
    const int seg0 = wave * 64 * rounds;

    for (int w = tid; w < fw + bw; w += W) field[w] = 0;  // (field and occ are adjacent)
    __syncthreads();
    if (tid == 0) set_pad_bits(occ, bw, C);
    __syncthreads();
    int rep = 0;
    for (int q = tid; q < Q; q += W) rep |= load_queen(queens, occ, in, N, q);
    __syncthreads();  // queens and occ are complete; every byte of state_in is read
    const bool repeated = block_sum<W>(rep, red) != 0;

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
            for (long long t = tid; t <= a.n_iters; t += W) hist[t] = e;
        if (tid == 0) store_eo3d_figures(a, ch, e, e, e, 0, 0, 0, 0, 0, 0, MCQ_EO3D_REPEATED);
        return;
    }

    for (int x = tid; x < Q * SLOTS; x += W) put_slot<W, BITS, STEPS>(field, queens, N, x);
    if (bs) store_queens(bs, queens, Q, tid, W);  // the best placement of a call without a new best is its input
    __syncthreads();
    int twoE = 0;
    for (int q = tid; q < Q; q += W) twoE += attackers_at<BITS>(field, N, queens[q]);
    const int e_in = block_sum<W>(twoE, red) >> 1;

    int E = e_in, B = e_in;
    if (a.best_floor) B = min(B, a.best_floor[ch]);
    long long moves = 0, uphill = 0, flat = 0, free_moves = 0, idle = 0, best_iter = 0;
    if (hist && tid == 0) hist[0] = E;

    for (long long t = 0; t < a.n_iters; t++) {
        if (E == 0) {  // (uniform: every lane holds the same E)
            idle++;
            if (hist && tid == 0) hist[t + 1] = E;
            continue;
        }
        uint32_t x0, x3;
        int oq, ot;
        eo3d_draw(seed, (unsigned long long)(a.first_iter + t), Q, C, x0, oq, ot, x3);

        // (2), (3): the bins cleared, j counted, lambda of every queen into the bins
        for (int b = tid; b < n_bins; b += W) bins[b] = 0;
        __syncthreads();
        int jc = 0;
        for (int i = tid; i < a.n_ranks; i += W) jc += a.rank_cdf[i] <= x0;
        int j = block_sum<W>(jc, red);
        j = min(j, Q - 1);  // (n_ranks <= Q - 1 already)
        for (int q = tid; q < Q; q += W) atomicAdd(&bins[attackers_at<BITS>(field, N, queens[q])], 1u);
        __syncthreads();

        // (4) the value class of position j, by every wavefront alike: lane l takes the bins n_bins - 1 - (l per_lane + i), worst first
        int s = 0;
        for (int i = 0; i < per_lane; i++) {
            const int x = lane * per_lane + i;
            s += x < n_bins ? (int)bins[n_bins - 1 - x] : 0;
        }
        const int incl = wave_scan(s);
        int found = -1, above_l = 0;
        if (j >= incl - s && j < incl) {  // one lane: the bins in front of its own hold at most j queens, with its own more
            int run = incl - s;
            for (int i = 0; i < per_lane; i++) {
                const int x = lane * per_lane + i;
                const int c = x < n_bins ? (int)bins[n_bins - 1 - x] : 0;
                if (found < 0 && run + c > j) found = n_bins - 1 - x, above_l = run;
                run += c;
            }
        }
        const int src = __ffsll(__ballot(found >= 0)) - 1;
        const int v = __shfl(found, src, 64), above = __shfl(above_l, src, 64);
        const int size = (int)bins[v];

        // (5) the queen: the members of the class per wavefront, then the walk of the wavefront that holds the ordinal
        int cnt = 0, lo = 0;
        for (int i = 0; i < rounds; i++) {
            const int q = seg0 + 64 * i + lane;
            const bool member = q < Q && attackers_at<BITS>(field, N, queens[q]) == v;
            cnt += __popcll(__ballot(member));
            lo += __popcll(__ballot(member && q < oq));
        }
        int before = 0, n_lo = lo;
        if (W > 64) {
            if (lane == 0) aux[wave] = (uint32_t)cnt | (uint32_t)lo << 16;  // both sums stay below 2^15
            __syncthreads();
            n_lo = 0;
            for (int w = 0; w < WAVES; w++) {
                const uint32_t x = aux[w];
                before += w < wave ? (int)(x & 0xFFFFu) : 0;
                n_lo += (int)(x >> 16);
            }
        }
        int want = j - above + n_lo;  // the ordinal in the order of rho_q, turned into the order of q
        want -= want >= size ? size : 0;
        if (want >= before && want < before + cnt) {  // (one wavefront; no barrier inside)
            int run = before;
            for (int i = 0; i < rounds; i++) {
                const int q = seg0 + 64 * i + lane;
                const bool member = q < Q && attackers_at<BITS>(field, N, queens[q]) == v;
                const unsigned long long b = __ballot(member);
                if (member && run + ballot_prefix(b) == want) aux[AUX_PICK] = (uint32_t)q;
                run += __popcll(b);
            }
        }
        __syncthreads();  // the pick is written, and every lane is done with the field of the placement
        const int q = (int)aux[AUX_PICK];
        const int p = queens[q];
        const int pcell = cell_of(p, N);

        // (6) the target, with the queen out of the field
        put<W, BITS, STEPS>(field, N, p, -1, tid, W, SLOTS);
        __syncthreads();
        int tcell, at;
        if (a.move == MCQ_EO3D_MOVE_BEST) {  // (uniform: an argument)
            uint32_t key = KEY_NONE;
            for (int w = tid; w < fw; w += W) {
                const uint32_t fv = field[w];
                const int c0 = w * CPD;
                const uint32_t o = occ[c0 >> 5] >> (c0 & 31);
#pragma unroll
                for (int b = 0; b < CPD; b++) {
                    if ((o >> b) & 1u) continue;  // a queen (the one that moves among them), or a pad bit
                    int rho = c0 + b - ot;
                    rho += rho < 0 ? C : 0;
                    key = min(key, ((fv >> (b * BITS)) & ((1u << BITS) - 1u)) << RHO_BITS | (uint32_t)rho);
                }
            }
            key = block_min<W, true>(key, red);
            at = (int)(key >> RHO_BITS);
            tcell = (int)(key & RHO_MASK) + ot;
            tcell -= tcell >= C ? C : 0;
        } else {
            const int m = eo3d_ordinal(x3, C - Q);
            const uint32_t z = tid < bw ? ~occ[tid] : 0u;  // the free cells of this lane's dword
            const int n = __popc(z);
            const int upto = wave_scan(n);
            int front = upto - n;
            if (W > 64) {
                if (lane == 63) aux[wave] = (uint32_t)upto;
                __syncthreads();
                for (int w = 0; w < WAVES; w++) front += w < wave ? (int)aux[w] : 0;
            }
            if (m >= front && m < front + n) {  // (one lane)
                uint32_t rest = z;
                for (int i = m - front; i; i--) rest &= rest - 1u;
                aux[AUX_PICK] = (uint32_t)(32 * tid + __ffs(rest) - 1);
            }
            __syncthreads();
            tcell = (int)aux[AUX_PICK];
            at = field_at<BITS>(field, tcell);
        }
        const int tp = packed_of(tcell, N, N2);
        const int delta = at - v;  // lambda(q) = v
        __syncthreads();  // every lane has read S(t) and the pick before the field and aux change
        put<W, BITS, STEPS>(field, N, tp, +1, tid, W, SLOTS);
        if (tid == 0) {
            vacate(occ, pcell);
            occupy(occ, queens, q, tp, tcell);
        }
        __syncthreads();
        moves++;
        uphill += delta > 0;
        flat += delta == 0;
        free_moves += v == 0;
        E += delta;
        if (E < B) {  // (uniform)
            B = E, best_iter = t + 1;
            if (bs) store_queens(bs, queens, Q, tid, W);
        }
        if (hist && tid == 0) hist[t + 1] = E;
    }
    __syncthreads();

    store_queens(out, queens, Q, tid, W);
    if (tid == 0) store_eo3d_figures(a, ch, e_in, E, B, best_iter, moves, uphill, flat, free_moves, idle, 0);
}

// the bytes of LDS of a chain: red, aux, the bins, the field, occ and the queens
long long lds_bytes(int N, int Q) {
    const long long cells = (long long)N * N * N, cpd = N <= 19 ? 4 : 2;
    return 4 * (EXTRA + (cells + cpd - 1) / cpd + (cells + 31) / 32 + ((long long)Q + 1) / 2);
}

// what both entry points refuse
int check_eo3d(const mcq_eo3d* q) {
    if (!q) return fail(g_eo3d_err, MCQ_EINVAL, "mcq_eo3d: NULL parameter block");
    const int rc = mcq_post::check_full3d(g_eo3d_err, "extremal optimisation", q->N, q->n_queens, (long long)q->n_chains);
    if (rc != MCQ_OK) return rc;
    const int Q = queens_of(q);
    if (q->n_iters < 0) return fail(g_eo3d_err, MCQ_EINVAL, "n_iters must be >= 0 (0 = the recount), got %lld", (long long)q->n_iters);
    if (q->first_iter < 0) return fail(g_eo3d_err, MCQ_EINVAL, "first_iter must be >= 0, got %lld", (long long)q->first_iter);
    if ((unsigned long long)q->first_iter + (unsigned long long)q->n_iters >= (1ull << 63))
        return fail(g_eo3d_err, MCQ_EINVAL, "iterations: first_iter + n_iters must stay below 2^63 (first_iter %lld, n_iters %lld)", (long long)q->first_iter,
                    (long long)q->n_iters);
    if (q->move != MCQ_EO3D_MOVE_BEST && q->move != MCQ_EO3D_MOVE_RANDOM)
        return fail(g_eo3d_err, MCQ_EINVAL, "move must be %d (best) or %d (random), got %d", MCQ_EO3D_MOVE_BEST, MCQ_EO3D_MOVE_RANDOM, (int)q->move);
    if (q->n_ranks < 0 || q->n_ranks > Q - 1) return fail(g_eo3d_err, MCQ_EINVAL, "n_ranks out of range [0, Q - 1 = %d]: %d", Q - 1, (int)q->n_ranks);
    if (q->n_ranks > 0 && !q->rank_cdf) return fail(g_eo3d_err, MCQ_EINVAL, "rank_cdf is required when n_ranks > 0 (n_ranks %d)", (int)q->n_ranks);
    if (!q->seeds) return fail(g_eo3d_err, MCQ_EINVAL, "seeds is required");
    if (!q->state_in) return fail(g_eo3d_err, MCQ_EINVAL, "state_in is required");
    if (!q->state_out) return fail(g_eo3d_err, MCQ_EINVAL, "state_out is required");
    if (q->energy_hist && q->hist_stride < q->n_iters + 1)
        return fail(g_eo3d_err, MCQ_EINVAL, "hist_stride must be >= n_iters + 1 = %lld, got %lld", (long long)q->n_iters + 1, (long long)q->hist_stride);
    if (q->best_state && (q->best_state == q->state_in || q->best_state == q->state_out))
        return fail(g_eo3d_err, MCQ_EINVAL, "best_state must be distinct from state_in and state_out (it is written while they are in use)");
    return MCQ_OK;
}

// chains first .. last - 1 through the rule: an int field per cell, and a stable sort of the queens in every iteration
void host_chains(const mcq_eo3d* q, long long first, long long last) {
    const int N = q->N, Q = queens_of(q);
    HostField f(N, Q);
    const std::vector<int>& S = f.S;
    const int C = f.C;
    std::vector<int> lam((size_t)Q), rho((size_t)Q), order((size_t)Q);
    for (long long ch = first; ch < last; ch++) {
        const bool repeated = f.load(q->state_in + ch * 3 * Q);
        const int e_in = f.energy();
        uint8_t* bs = q->best_state ? q->best_state + ch * 3 * Q : nullptr;
        int32_t* hist = q->energy_hist ? q->energy_hist + ch * q->hist_stride : nullptr;
        if (bs) f.store(bs);
        if (repeated) {
            f.store(q->state_out + ch * 3 * Q);
            if (hist)
                for (long long t = 0; t <= q->n_iters; t++) hist[t] = e_in;
            store_eo3d_figures(*q, ch, e_in, e_in, e_in, 0, 0, 0, 0, 0, 0, MCQ_EO3D_REPEATED);
            continue;
        }
        int E = e_in, B = e_in;
        if (q->best_floor && q->best_floor[ch] < B) B = q->best_floor[ch];
        long long moves = 0, uphill = 0, flat = 0, free_moves = 0, idle = 0, best_iter = 0;
        if (hist) hist[0] = E;
        const uint32_t seed = q->seeds[ch];
        for (long long t = 0; t < q->n_iters; t++) {
            if (E == 0) {
                idle++;
                if (hist) hist[t + 1] = E;
                continue;
            }
            uint32_t x0, x3;
            int oq, ot;
            eo3d_draw(seed, (unsigned long long)(q->first_iter + t), Q, C, x0, oq, ot, x3);
            int j = 0;
            for (int i = 0; i < q->n_ranks; i++) j += q->rank_cdf[i] <= x0;
            for (int n = 0; n < Q; n++) {
                lam[(size_t)n] = S[(size_t)f.pos[(size_t)n]] - 1;
                rho[(size_t)n] = (n - oq + Q) % Q;
                order[(size_t)n] = n;
            }
            std::stable_sort(order.begin(), order.end(), [&](int n1, int n2) {
                if (lam[(size_t)n1] != lam[(size_t)n2]) return lam[(size_t)n1] > lam[(size_t)n2];  // the worst first
                return rho[(size_t)n1] < rho[(size_t)n2];
            });
            const int n = order[(size_t)j], p = f.pos[(size_t)n], v = lam[(size_t)n];
            f.take_out(n);  // S is a(n, .) now; the cell p reads as free from here on, and is none
            int cell = -1;
            if (q->move == MCQ_EO3D_MOVE_BEST) {
                int ba = INT_MAX, br = INT_MAX;
                for (int c = 0; c < C; c++) {
                    if (f.occ[(size_t)c] || c == p) continue;
                    const int r = (c - ot + C) % C;
                    if (S[(size_t)c] < ba || (S[(size_t)c] == ba && r < br)) ba = S[(size_t)c], br = r, cell = c;
                }
            } else {
                int left = eo3d_ordinal(x3, C - Q);
                for (int c = 0; c < C && cell < 0; c++) {
                    if (f.occ[(size_t)c] || c == p) continue;
                    if (left-- == 0) cell = c;
                }
            }
            const int delta = S[(size_t)cell] - v;
            f.put_back(n, cell);
            moves++;
            uphill += delta > 0;
            flat += delta == 0;
            free_moves += v == 0;
            E += delta;
            if (E < B) {
                B = E, best_iter = t + 1;
                if (bs) f.store(bs);
            }
            if (hist) hist[t + 1] = E;
        }
        f.store(q->state_out + ch * 3 * Q);
        store_eo3d_figures(*q, ch, e_in, E, B, best_iter, moves, uphill, flat, free_moves, idle, 0);
    }
}

}  // namespace

extern "C" {

const char* mcq_eo3d_last_error(void) { return g_eo3d_err; }

int mcq_eo3d_host(const mcq_eo3d* q) {
    const int rc = check_eo3d(q);
    if (rc != MCQ_OK) return rc;
    for (int i = 1; i < q->n_ranks; i++)
        if (q->rank_cdf[i] < q->rank_cdf[i - 1])
            return fail(g_eo3d_err, MCQ_EINVAL, "rank_cdf must not decrease: entry %d is %u behind %u", i, (unsigned)q->rank_cdf[i], (unsigned)q->rank_cdf[i - 1]);
    mcq_post::for_chains((long long)q->n_chains, [q](long long first, long long last) { host_chains(q, first, last); });
    return MCQ_OK;
}

int mcq_eo3d_device(const mcq_eo3d* q, void* hip_stream) {
    const int rc = check_eo3d(q);
    if (rc != MCQ_OK) return rc;
    const int Q = queens_of(q);
    const long long bytes = lds_bytes(q->N, Q);
    if (bytes > MCQ_MAX_EO3D_LDS)  // (no shape in range is: 137 088 bytes at N = 32 with Q = N^3 - 1)
        return fail(g_eo3d_err, MCQ_EINVAL, "N = %d with n_queens = %d: a chain takes %lld bytes of LDS, above the %d of a workgroup", (int)q->N, Q, bytes,
                    MCQ_MAX_EO3D_LDS);
    hipStream_t s = (hipStream_t)hip_stream;
    const Eo3dArgs a{q->seeds, q->rank_cdf, q->state_in, q->state_out, q->best_floor, q->energy_in, q->energy_out, q->best_energy, q->best_iter,
                     q->best_state, q->n_moves, q->n_uphill, q->n_flat, q->n_free, q->n_idle, q->energy_hist, q->flags, (long long)q->hist_stride,
                     (long long)q->n_iters, (long long)q->first_iter, (int)q->move, (int)q->n_ranks, (int)q->N, Q};
    const hipError_t e = for_shape_of(a.N, [&](auto shape) {
        using S = decltype(shape);
        return launch<S>(mcq_eo3d_kernel<S::W, S::BITS, S::STEPS>, a, a.N, a.Q, EXTRA, (long long)q->n_chains, s);
    });
    if (e != hipSuccess) return fail(g_eo3d_err, MCQ_EDEVICE, "mcq_eo3d_device: %s", hipGetErrorString(e));
    return MCQ_OK;
}

}  // extern "C"
