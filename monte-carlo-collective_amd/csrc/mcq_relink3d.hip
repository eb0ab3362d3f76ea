// mcq_relink3d.hip -- path relinking between full_3d placements: walk from a placement towards a guide, one queen at a time, always the
// cheapest remaining (queen, cell) pair, and hand the best placement met on the way to the local search (include/mcq.h: mcq_relink3d,
// where the rule is stated).  The field, its update and the start of a chain are those of csrc/mcq_field.h; the descent and the restore
// are those of csrc/mcq_hop3d.hip, restated here so that file stays as it is; what this file adds is the walk between two placements,
// as one launch.
//
//   kernel  one chain per workgroup of W lanes, all in LDS: red, 32 dwords; gocc, the bitmap of the guide's cells; then the field S of
//           the WHOLE placement, occ and the queens (csrc/mcq_field.h); behind them pbest, Q more packed cells (the best placement of the
//           path, the clamped input to begin with), and the two lists mlist (the moving queens' indices) and tlist (the open targets,
//           packed), D = min(Q, N^3 - Q) 16-bit entries each.  The field is built ONCE per launch.
//           LISTS: a queen whose cell is not in gocc joins mlist, a cell of gocc & ~occ joins tlist, each through a counter in red (an
//           LDS atomic): the order within a list is free, the key decides.  Both counters end on d0.
//           STEP: with m entries left, the m^2 pairs x = i m + j are spread over the lanes, (i, j) advanced by (W / m, W % m) with one
//           carry, so a short walk keeps the lanes as busy as a long one.  A pair reads S(c) and S(pos(q)), tests [pos(q) attacks c] and
//           forms the 64-bit key (delta + 403) << 30 | rho_q << 15 | rho_t; block_min64 picks the smallest.  Keys of different pairs
//           differ, so exactly one lane holds the winner: behind a barrier all lanes put -1 on the lines of the cell left and +1 on those
//           of the cell taken, and that lane updates occ, queens and the two lists (its entries swapped with the last ones).  On a
//           candidate with a new low the queens are copied to pbest.
//           BACK: the restore of csrc/mcq_hop3d.hip on the queens with queens[q] != pbest[q]; then its descent.
//           BARRIERS: every branch around a barrier is taken on values that every lane computed alike from the arguments (n_steps, t,
//           m, the candidate window), read from red behind a barrier (the repeat flags, d0, the winning key, a pass's minimum) or
//           carries along from such values (E, best_e, moved, lp): the repeat exit, the end of the walk, a new low, the queen skipped
//           by the descent and the descent's end are all uniform over the workgroup, so every barrier is reached by all lanes.  The
//           one branch that is NOT uniform, `key == best`, holds no barrier.
//   host    mcq_relink3d_host: the same rule on HostField with plain loops and tuple comparisons, for every shape.
//
// Built for gfx950 only, with csrc/mcq_hip.hip:  hipcc --offload-arch=gfx950 -O3 -ffp-contract=off
#include <hip/hip_runtime.h>

#include <climits>
#include <vector>

#include "../../include/mcq.h"
#include "mcq_field.h"
#include "mcq_post.h"

namespace {

using namespace mcq_field;
using mcq_post::fail;
using mcq_post::queens_of;

thread_local char g_relink3d_err[256] = "";

constexpr uint32_t RELINK3D_KEY_WORD = 10u;  // key word 1 of the chain's Philox stream: 0 - 9 are taken (include/mcq.h: mcq_relink3d, item 2)
constexpr int RHO_BITS = 15;                 // rho_q < Q < 32^3 and rho_t < N^3 <= 32^3
constexpr int DELTA_BIAS = 13 * (MCQ_MAX_N_QUENCH3D - 1);  // 403: |delta| <= 13 (N - 1), so 0 <= delta + DELTA_BIAS <= 806 < 2^10
constexpr uint32_t RHO_MASK = (1u << RHO_BITS) - 1u;
constexpr unsigned long long KEY64_NONE = ~0ull;  // a pair's key stays below 2^40

struct Relink3dArgs {
    const uint32_t* seeds;
    const uint8_t* state_in;
    const uint8_t* guide_in;
    uint8_t* state_out;
    uint8_t* path_best_state;
    int32_t* distance_in;
    int32_t* n_steps;
    int32_t* path_best_step;
    int32_t* energy_in;
    int32_t* path_best_energy;
    int32_t* path_max_energy;
    int32_t* energy_out;
    int64_t* n_moves;
    int64_t* n_passes;
    int32_t* energy_hist;
    int32_t* flags;
    long long hist_stride;
    long long walk;
    int max_steps;
    int min_dist;
    int N;
    int Q;
};

// the per-chain figures, by one lane or by the host: `a` is the kernel's argument struct or the parameter block
template <class A>
__host__ __device__ __forceinline__ void store_relink3d_figures(const A& a, long long ch, int d0, int n_steps, int best_step, int e_in, int best_e,
                                                                int e_max, int E, long long moves, long long passes, int flags) {
    if (a.distance_in) a.distance_in[ch] = d0;
    if (a.n_steps) a.n_steps[ch] = n_steps;
    if (a.path_best_step) a.path_best_step[ch] = best_step;
    if (a.energy_in) a.energy_in[ch] = e_in;
    if (a.path_best_energy) a.path_best_energy[ch] = best_e;
    if (a.path_max_energy) a.path_max_energy[ch] = e_max;
    if (a.energy_out) a.energy_out[ch] = E;
    if (a.n_moves) a.n_moves[ch] = moves;
    if (a.n_passes) a.n_passes[ch] = passes;
    if (a.flags) a.flags[ch] = flags;
}

// the tie offsets of step t of walk `walk`: words 0 and 1 of philox4x32-10(counter = (t, walk low, walk high, 0), key = (seed, 10))
__host__ __device__ __forceinline__ void relink3d_draw(uint32_t seed, uint32_t t, unsigned long long walk, int Q, int C, int& oq, int& ot) {
    uint32_t c0 = t, c1 = (uint32_t)walk, c2 = (uint32_t)(walk >> 32), c3 = 0, k0 = seed, k1 = RELINK3D_KEY_WORD;
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1, c3 = (uint32_t)p0, c0 = n0, c2 = n2;
        k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
    }
    oq = (int)(((unsigned long long)c0 * (unsigned)Q) >> 32);
    ot = (int)(((unsigned long long)c1 * (unsigned)C) >> 32);
}

// whether the placement behind step t (counted from 1) is a candidate: rule item 3
__host__ __device__ __forceinline__ bool is_candidate(int t, int d0, int min_dist) { return t >= (min_dist > 1 ? min_dist : 1) && d0 - t >= min_dist; }

// the entries of a list: d0 is at most the queens and at most the free cells
__host__ __device__ __forceinline__ int list_len(int Q, int C) { return Q < C - Q ? Q : C - Q; }

// the minimum of a 64-bit key over the workgroup, through red as W / 64 pairs of dwords (all 32 at W = 1024)
template <int W>
__device__ __forceinline__ unsigned long long block_min64(unsigned long long v, uint32_t* red) {
    for (int o = 32; o; o >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o, 64);
        const unsigned long long other = (unsigned long long)hi << 32 | lo;
        v = other < v ? other : v;
    }
    if (W == 64) return v;
    __syncthreads();  // the readers of the reduction before this one are done with red
    if ((threadIdx.x & 63) == 0) red[2 * (threadIdx.x >> 6)] = (uint32_t)v, red[2 * (threadIdx.x >> 6) + 1] = (uint32_t)(v >> 32);
    __syncthreads();
    v = (unsigned long long)red[1] << 32 | red[0];
    for (int w = 1; w < W / 64; w++) {
        const unsigned long long other = (unsigned long long)red[2 * w + 1] << 32 | red[2 * w];
        v = other < v ? other : v;
    }
    return v;
}

// queen q of the guide, clamped to N - 1, into the guide's bitmap; true where the cell was taken already (a repeated guide)
__device__ __forceinline__ int load_guide(uint32_t* gocc, const uint8_t* gin, int N, int q) {
    const int i = min((int)gin[3 * q], N - 1), j = min((int)gin[3 * q + 1], N - 1), k = min((int)gin[3 * q + 2], N - 1);
    const int cell = (i * N + j) * N + k;
    const uint32_t bit = 1u << (cell & 31);
    return (atomicOr(&gocc[cell >> 5], bit) & bit) != 0;
}

template <int W, int BITS, int STEPS>
__global__ __launch_bounds__(W) void mcq_relink3d_kernel(Relink3dArgs a) {
    extern __shared__ uint32_t lds[];
    constexpr int CPD = 32 / BITS, SLOTS = 13 * STEPS;
    const int N = a.N, Q = a.Q, N2 = N * N, C = N2 * N;
    const int gbw = (C + 31) / 32, D = list_len(Q, C);
    uint32_t* red = lds;
    uint32_t* const gocc = lds + 32;
    const Chain chain = carve<BITS>(lds + 32 + gbw, C);
    uint32_t* const field = chain.field;
    uint32_t* const occ = chain.occ;
    uint16_t* const queens = chain.queens;
    uint16_t* const pbest = queens + 2 * ((Q + 1) / 2);  // behind the queens, on a dword; so are the two lists
    uint16_t* const mlist = pbest + 2 * ((Q + 1) / 2);
    uint16_t* const tlist = mlist + 2 * ((D + 1) / 2);
    const int fw = chain.fw, bw = chain.bw;
    const int tid = threadIdx.x;
    const long long ch = blockIdx.x;
    const uint32_t seed = a.seeds[ch];
    const uint8_t* in = a.state_in + ch * 3 * Q;
    const uint8_t* gin = a.guide_in + ch * 3 * Q;
    uint8_t* out = a.state_out + ch * 3 * Q;
    uint8_t* bs = a.path_best_state ? a.path_best_state + ch * 3 * Q : nullptr;
    int32_t* hist = a.energy_hist ? a.energy_hist + ch * a.hist_stride : nullptr;
    const int Wd = a.max_steps == 0 ? Q : a.max_steps;  // W of rule item 5

    for (int w = tid; w < gbw; w += W) gocc[w] = 0;
    for (int w = tid; w < fw + bw; w += W) field[w] = 0;  // (field and occ are adjacent)
    __syncthreads();
    if (tid == 0) set_pad_bits(occ, bw, C);
    __syncthreads();
    int rep = 0;
    for (int q = tid; q < Q; q += W) {
        rep += load_queen(queens, occ, in, N, q);
        rep += load_guide(gocc, gin, N, q) << 16;  // (a lane loads at most Q / W + 1 < 2^16 queens)
        pbest[q] = queens[q];
    }
    __syncthreads();  // queens, pbest, occ and gocc are complete; every byte of state_in and guide_in is read
    const int reps = block_sum<W>(rep, red);  // at most Q < 2^15 in either half
    const int flags = ((reps & 0xFFFF) ? MCQ_RELINK3D_REPEATED : 0) | ((reps >> 16) ? MCQ_RELINK3D_GUIDE_REPEATED : 0);

    if (flags) {  // rule item 6: recounted pair by pair, handed back unmoved (uniform: every lane read the same sums)
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
            for (int t = tid; t <= Wd; t += W) hist[t] = e;
        if (tid == 0) store_relink3d_figures(a, ch, 0, 0, 0, e, e, e, e, 0, 0, flags);
        return;
    }

    for (int x = tid; x < Q * SLOTS; x += W) put_slot<W, BITS, STEPS>(field, queens, N, x);
    __syncthreads();
    int twoE = 0;
    for (int q = tid; q < Q; q += W) twoE += attackers_at<BITS>(field, N, queens[q]);
    const int e_in = block_sum<W>(twoE, red) >> 1;

    // the lists of M and T, through two counters in red
    __syncthreads();  // the readers of the sum are done with red
    if (tid == 0) red[0] = 0, red[1] = 0;
    __syncthreads();
    for (int q = tid; q < Q; q += W) {
        const int cell = cell_of(queens[q], N);
        if (!((gocc[cell >> 5] >> (cell & 31)) & 1u)) {
            const int s = (int)atomicAdd(&red[0], 1u);
            if (s < D) mlist[s] = (uint16_t)q;  // (s >= D cannot happen -- |M| <= min(Q, N^3 - Q) --: it only keeps a broken rule inside the arrays)
        }
    }
    for (int w = tid; w < gbw; w += W) {
        uint32_t bits = gocc[w] & ~occ[w];  // (occ's pad bits are set, gocc's are not)
        while (bits) {
            const int b = __ffs((int)bits) - 1;
            bits &= bits - 1;
            const int s = (int)atomicAdd(&red[1], 1u);
            if (s < D) tlist[s] = (uint16_t)packed_of(w * 32 + b, N, N2);
        }
    }
    __syncthreads();
    const int d0 = min(min((int)red[0], (int)red[1]), D);  // (red[0] = red[1] <= D: neither placement is repeated; the minimum only keeps a broken rule inside the lists)
    __syncthreads();  // every lane has read the counters before a reduction writes red

    int E = e_in, e_max = e_in, best_e = INT_MAX, best_step = 0;
    const int n_steps = a.max_steps == 0 ? d0 : min(d0, a.max_steps);
    if (hist && tid == 0) hist[0] = E;

    // the walk
    for (int t = 0; t < n_steps; t++) {
        const int m = d0 - t;  // entries left in either list
        int oq, ot;
        relink3d_draw(seed, (uint32_t)t, (unsigned long long)a.walk, Q, C, oq, ot);
        unsigned long long key = KEY64_NONE;
        int bi = 0, bj = 0;
        const int wd = W / m, wm = W - wd * m;  // the lane's next pair is W further: (i, j) += (W / m, W % m), one carry
        int i = tid / m, j = tid - i * m;
        while (i < m) {
            const int q = mlist[i], p = queens[q], tp = tlist[j];
            const int tcell = cell_of(tp, N);
            const int delta = field_at<BITS>(field, tcell) - (int)attacks(p, tp) - (field_at<BITS>(field, cell_of(p, N)) - 1);
            int rq = q - oq, rt = tcell - ot;
            rq += rq < 0 ? Q : 0;
            rt += rt < 0 ? C : 0;
            const unsigned long long k = (unsigned long long)(uint32_t)(delta + DELTA_BIAS) << (2 * RHO_BITS) | (unsigned long long)(uint32_t)rq << RHO_BITS | (uint32_t)rt;
            if (k < key) key = k, bi = i, bj = j;
            i += wd, j += wm;
            if (j >= m) j -= m, i++;
        }
        const unsigned long long best = block_min64<W>(key, red);
        if (best == KEY64_NONE) break;  // (cannot happen -- m >= 1 pairs are left --: it only keeps a broken rule inside the arrays; uniform)
        const int delta = (int)(best >> (2 * RHO_BITS)) - DELTA_BIAS;
        int q = (int)((best >> RHO_BITS) & RHO_MASK) + oq;
        q -= q >= Q ? Q : 0;
        int tcell = (int)(best & RHO_MASK) + ot;
        tcell -= tcell >= C ? C : 0;
        const int p = queens[q];
        const int pcell = cell_of(p, N);
        const int tp = packed_of(tcell, N, N2);
        __syncthreads();  // every lane has read queens[q], the lists and the field before the queen moves
        put<W, BITS, STEPS>(field, N, p, -1, tid, W, SLOTS);
        put<W, BITS, STEPS>(field, N, tp, +1, tid, W, SLOTS);
        if (key == best) {  // ONE lane: the keys of different pairs differ.  No barrier inside
            vacate(occ, pcell);
            occupy(occ, queens, q, tp, tcell);
            mlist[bi] = mlist[m - 1];
            tlist[bj] = tlist[m - 1];
        }
        __syncthreads();
        E += delta;
        e_max = max(e_max, E);
        if (is_candidate(t + 1, d0, a.min_dist) && E < best_e) {  // (uniform; the next write of queens lies behind the next step's barrier)
            best_e = E, best_step = t + 1;
            for (int qq = tid; qq < Q; qq += W) pbest[qq] = queens[qq];
        }
        if (hist && tid == 0) hist[t + 1] = E;
    }
    if (hist)
        for (int t = n_steps + 1 + tid; t <= Wd; t += W) hist[t] = E;
    if (best_step == 0) best_e = e_in;  // no candidate: P* is the clamped input, which pbest still holds

    // back to P*: the restore of csrc/mcq_hop3d.hip on the queens that moved behind it
    __syncthreads();
    for (int q = tid; q < Q; q += W) {
        const int cur = queens[q];
        if (cur != pbest[q]) {
            const int c = cell_of(cur, N);
            atomicAnd(&occ[c >> 5], ~(1u << (c & 31)));
        }
    }
    __syncthreads();  // every bit of a cell that is left is cleared before a bit of a cell that is taken again is set
    for (int q = tid; q < Q; q += W) {
        const int old = pbest[q];
        if (old != queens[q]) {
            const int c = cell_of(old, N);
            atomicOr(&occ[c >> 5], 1u << (c & 31));
        }
    }
    for (int x = tid; x < Q * SLOTS; x += W) {
        const int q = x / SLOTS, s = x - q * SLOTS;
        const int cur = queens[q], old = pbest[q];
        if (cur != old) {
            put<W, BITS, STEPS>(field, N, cur, -1, s, SLOTS, SLOTS);
            put<W, BITS, STEPS>(field, N, old, +1, s, SLOTS, SLOTS);
        }
    }
    __syncthreads();  // every lane has compared queens with pbest
    for (int q = tid; q < Q; q += W) queens[q] = pbest[q];
    E = best_e;
    __syncthreads();  // the field, occ and the queens are P*'s

    // the descent: the pass loop of csrc/mcq_quench3d.hip, as csrc/mcq_hop3d.hip runs it
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

    __syncthreads();
    store_queens(out, queens, Q, tid, W);
    if (bs) store_queens(bs, pbest, Q, tid, W);
    if (tid == 0) store_relink3d_figures(a, ch, d0, n_steps, best_step, e_in, best_e, e_max, E, (long long)lm, (long long)lp, 0);
}

// W of rule item 5: the last entry of a chain's history
long long hist_width(const mcq_relink3d* q) { return q->max_steps == 0 ? (long long)queens_of(q) : (long long)q->max_steps; }

// what both entry points refuse
int check_relink3d(const mcq_relink3d* q) {
    if (!q) return fail(g_relink3d_err, MCQ_EINVAL, "mcq_relink3d: NULL parameter block");
    const int rc = mcq_post::check_full3d(g_relink3d_err, "path relinking", q->N, q->n_queens, (long long)q->n_chains);
    if (rc != MCQ_OK) return rc;
    const int Q = queens_of(q);
    if (q->max_steps < 0 || q->max_steps > Q)
        return fail(g_relink3d_err, MCQ_EINVAL, "max_steps out of range [0, Q = %d] (0 = the whole way to the guide): %d", Q, (int)q->max_steps);
    if (q->min_dist < 0 || q->min_dist > Q) return fail(g_relink3d_err, MCQ_EINVAL, "min_dist out of range [0, Q = %d]: %d", Q, (int)q->min_dist);
    if (q->walk < 0) return fail(g_relink3d_err, MCQ_EINVAL, "walk must be >= 0, got %lld", (long long)q->walk);
    if (!q->seeds) return fail(g_relink3d_err, MCQ_EINVAL, "seeds is required");
    if (!q->state_in) return fail(g_relink3d_err, MCQ_EINVAL, "state_in is required");
    if (!q->guide_in) return fail(g_relink3d_err, MCQ_EINVAL, "guide_in is required");
    if (!q->state_out) return fail(g_relink3d_err, MCQ_EINVAL, "state_out is required");
    if (q->state_out == q->guide_in) return fail(g_relink3d_err, MCQ_EINVAL, "state_out must be distinct from guide_in (it may be state_in)");
    if (q->path_best_state && (q->path_best_state == q->state_in || q->path_best_state == q->guide_in || q->path_best_state == q->state_out))
        return fail(g_relink3d_err, MCQ_EINVAL, "path_best_state must be distinct from state_in, guide_in and state_out");
    if (q->energy_hist && q->hist_stride < hist_width(q) + 1)
        return fail(g_relink3d_err, MCQ_EINVAL, "hist_stride must be >= W + 1 = %lld (W = max_steps, or Q when that is 0), got %lld", hist_width(q) + 1,
                    (long long)q->hist_stride);
    return MCQ_OK;
}

// the dwords of a chain in front of the field (red, gocc) and behind the queens (pbest, mlist, tlist): `extra` of mcq_field::launch
int extra_dwords(int N, int Q) {
    const int cells = N * N * N, D = list_len(Q, cells);
    return 32 + (cells + 31) / 32 + (Q + 1) / 2 + 2 * ((D + 1) / 2);
}

// the bytes of LDS of a chain: red, gocc, the field, occ, the queens, pbest and the two lists
long long lds_bytes(int N, int Q) {
    const long long cells = (long long)N * N * N, cpd = N <= 19 ? 4 : 2;
    return 4 * (extra_dwords(N, Q) + (cells + cpd - 1) / cpd + (cells + 31) / 32 + ((long long)Q + 1) / 2);
}

// a packed cell from its index (host)
inline int host_packed(int cell, int N, int N2) { return (cell / N2) << 10 | ((cell / N) % N) << 5 | (cell % N); }

// chains first .. last - 1 through the rule, with an int field per cell
void host_chains(const mcq_relink3d* q, long long first, long long last) {
    const int N = q->N, Q = queens_of(q);
    HostField f(N, Q);
    const std::vector<int>& S = f.S;
    const int C = f.C, N2 = f.N2;
    std::vector<uint8_t> gocc((size_t)C);
    std::vector<int> pbest((size_t)Q), mq, tc;
    const long long W = hist_width(q);
    for (long long ch = first; ch < last; ch++) {
        const bool repeated = f.load(q->state_in + ch * 3 * Q);
        const int e_in = f.energy();
        const uint8_t* gin = q->guide_in + ch * 3 * Q;
        bool guide_repeated = false;
        for (int c = 0; c < C; c++) gocc[(size_t)c] = 0;
        for (int n = 0; n < Q; n++) {
            const int i = gin[3 * n] < N ? gin[3 * n] : N - 1, j = gin[3 * n + 1] < N ? gin[3 * n + 1] : N - 1, k = gin[3 * n + 2] < N ? gin[3 * n + 2] : N - 1;
            const int cell = (i * N + j) * N + k;
            guide_repeated |= gocc[(size_t)cell] != 0;
            gocc[(size_t)cell] = 1;
        }
        uint8_t* bs = q->path_best_state ? q->path_best_state + ch * 3 * Q : nullptr;
        int32_t* hist = q->energy_hist ? q->energy_hist + ch * q->hist_stride : nullptr;
        const int flags = (repeated ? MCQ_RELINK3D_REPEATED : 0) | (guide_repeated ? MCQ_RELINK3D_GUIDE_REPEATED : 0);
        if (flags) {
            f.store(q->state_out + ch * 3 * Q);
            if (bs) f.store(bs);
            if (hist)
                for (long long t = 0; t <= W; t++) hist[t] = e_in;
            store_relink3d_figures(*q, ch, 0, 0, 0, e_in, e_in, e_in, e_in, 0, 0, flags);
            continue;
        }
        mq.clear(), tc.clear();
        for (int n = 0; n < Q; n++)
            if (!gocc[(size_t)f.pos[(size_t)n]]) mq.push_back(n);
        for (int c = 0; c < C; c++)
            if (gocc[(size_t)c] && !f.occ[(size_t)c]) tc.push_back(c);
        const int d0 = (int)mq.size();
        const int n_steps = q->max_steps == 0 ? d0 : (d0 < q->max_steps ? d0 : q->max_steps);
        int E = e_in, e_max = e_in, best_e = INT_MAX, best_step = 0;
        pbest = f.pos;
        if (hist) hist[0] = E;
        const uint32_t seed = q->seeds[ch];
        for (int t = 0; t < n_steps; t++) {
            int oq, ot;
            relink3d_draw(seed, (uint32_t)t, (unsigned long long)q->walk, Q, C, oq, ot);
            int bd = INT_MAX, brq = 0, brt = 0;
            size_t bi = 0, bj = 0;
            for (size_t i = 0; i < mq.size(); i++) {
                const int n = mq[i], p = f.pos[(size_t)n], pp = host_packed(p, N, N2), base = S[(size_t)p] - 1;
                const int rq = n - oq + (n < oq ? Q : 0);
                for (size_t j = 0; j < tc.size(); j++) {
                    const int c = tc[j];
                    const int delta = S[(size_t)c] - (int)attacks(pp, host_packed(c, N, N2)) - base;
                    const int rt = c - ot + (c < ot ? C : 0);
                    if (delta < bd || (delta == bd && (rq < brq || (rq == brq && rt < brt)))) bd = delta, brq = rq, brt = rt, bi = i, bj = j;
                }
            }
            const int n = mq[bi], c = tc[bj];
            f.take_out(n);
            f.put_back(n, c);
            mq[bi] = mq.back(), mq.pop_back();
            tc[bj] = tc.back(), tc.pop_back();
            E += bd;
            if (E > e_max) e_max = E;
            if (is_candidate(t + 1, d0, q->min_dist) && E < best_e) best_e = E, best_step = t + 1, pbest = f.pos;
            if (hist) hist[t + 1] = E;
        }
        if (hist)
            for (long long t = n_steps + 1; t <= W; t++) hist[t] = E;
        if (best_step == 0) best_e = e_in;

        // back to P*: every queen that moved behind it leaves, then every one of them returns
        for (int n = 0; n < Q; n++)
            if (f.pos[(size_t)n] != pbest[(size_t)n]) f.take_out(n);
        for (int n = 0; n < Q; n++)
            if (f.pos[(size_t)n] != pbest[(size_t)n]) f.put_back(n, pbest[(size_t)n]);
        if (bs) f.store(bs);
        E = best_e;

        // L: passes of the quench rule until one moves nothing
        long long moves = 0, passes = 0;
        for (;;) {
            int moved = 0;
            for (int n = 0; n < Q; n++) {
                const int p = f.pos[(size_t)n], now = S[(size_t)p] - 1;
                if (now == 0) continue;  // no cell can hold less
                f.take_out(n);
                int t = -1;
                for (int c = 0; c < C; c++)
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
        f.store(q->state_out + ch * 3 * Q);
        store_relink3d_figures(*q, ch, d0, n_steps, best_step, e_in, best_e, e_max, E, moves, passes, 0);
    }
}

}  // namespace

extern "C" {

const char* mcq_relink3d_last_error(void) { return g_relink3d_err; }

int mcq_relink3d_host(const mcq_relink3d* q) {
    const int rc = check_relink3d(q);
    if (rc != MCQ_OK) return rc;
    mcq_post::for_chains((long long)q->n_chains, [q](long long first, long long last) { host_chains(q, first, last); });
    return MCQ_OK;
}

int mcq_relink3d_device(const mcq_relink3d* q, void* hip_stream) {
    const int rc = check_relink3d(q);
    if (rc != MCQ_OK) return rc;
    const int Q = queens_of(q);
    const long long bytes = lds_bytes(q->N, Q);
    if (bytes > MCQ_MAX_RELINK3D_LDS)
        return fail(g_relink3d_err, MCQ_EINVAL, "N = %d with n_queens = %d: a chain takes %lld bytes of LDS, above the %d of a workgroup "
                    "(mcq_relink3d_device runs every Q = N^2; mcq_relink3d_host runs every shape)", (int)q->N, Q, bytes, MCQ_MAX_RELINK3D_LDS);
    hipStream_t s = (hipStream_t)hip_stream;
    const Relink3dArgs a{q->seeds, q->state_in, q->guide_in, q->state_out, q->path_best_state, q->distance_in, q->n_steps, q->path_best_step,
                         q->energy_in, q->path_best_energy, q->path_max_energy, q->energy_out, q->n_moves, q->n_passes, q->energy_hist, q->flags,
                         (long long)q->hist_stride, (long long)q->walk, (int)q->max_steps, (int)q->min_dist, (int)q->N, Q};
    const int extra = extra_dwords(a.N, a.Q);
    const hipError_t e = for_shape_of(a.N, [&](auto shape) {
        using S = decltype(shape);
        return launch<S>(mcq_relink3d_kernel<S::W, S::BITS, S::STEPS>, a, a.N, a.Q, extra, (long long)q->n_chains, s);
    });
    if (e != hipSuccess) return fail(g_relink3d_err, MCQ_EDEVICE, "mcq_relink3d_device: %s", hipGetErrorString(e));
    return MCQ_OK;
}

}  // extern "C"
