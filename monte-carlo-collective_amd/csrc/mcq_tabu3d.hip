// mcq_tabu3d.hip -- tabu search of full_3d placements: every iteration takes the best admissible move of a conflicting queen to a free
// cell of the cube, also when it raises the energy, and forbids the cell it left for a while (include/mcq.h: mcq_tabu3d, where the rule
// is stated).  The field, its update and the start of a chain are those of csrc/mcq_field.h; the stamp base is that of csrc/mcq_tabu.hip,
// which both files take from csrc/mcq_post.h.
//
//   kernel  one chain per workgroup of W lanes, all in LDS: red, 32 dwords; the stamps T(t), one uint16 per cell, relative to a base
//           that moves by 2^15 every 2^15 iterations; then the field S of the WHOLE placement, occ and the queens (csrc/mcq_field.h).
//           The field is built ONCE per launch; a move puts -1 on the lines of the cell left and +1 on those of the cell taken, and no
//           queen is ever taken out of the field during an iteration.  For a free cell t, a(q, t) = S(t) - [pos(q) attacks t], and
//           a(q, pos(q)) = S(pos(q)) - 1.
//           ITERATION: (1) a pass over the cube, a dword of the field and its cells' stamps (one or two dwords) per lane and step: the smallest (S(t), rho_t) over the free cells
//           that are not tabu, G_free, and over the free cells that are, G_tabu, as keys S << 15 | rho_t.  (2) a pass over the queens, a
//           queen per lane and step: a conflicting queen with c = a(q, pos(q)) walks the <= 13 (N - 1) cells on its lines for the
//           smallest (S(t) - 1, rho_t) over the free cells that are not tabu or have S(t) - 1 < T_q = B - E + c (aspiration), L_q; its
//           best target is the smallest of G_free, G_tabu when G_tabu's S < T_q, and L_q.  G counts a line cell of the queen one too
//           high, so whenever such a cell would win G the same cell in L_q beats it by one; and when the smallest tabu cell of G_tabu
//           has S >= T_q no tabu cell off the lines is admissible.  (3) the winner over the queens is the smallest 64-bit key
//           (delta + DELTA_BIAS) << 30 | rho_q << 15 | rho_t.  (4) the move: one stamp store, the two updates of the field, E, the
//           counters, and best_state to global memory when B falls.
//           Every branch around a barrier (the stamp base's move, a stalled iteration, the move, B falling) is taken on values that
//           every lane computed alike from the arguments or read from `red` behind a barrier, so every barrier is reached by all lanes.
//   host    mcq_tabu3d_host: the same rule on HostField with plain loops and absolute 64-bit stamps, for every shape.
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
using mcq_post::rebase2;
using mcq_post::REBASE;

thread_local char g_tabu3d_err[256] = "";

constexpr uint32_t TABU3D_KEY_WORD = 8u;  // key word 1 of the chain's Philox stream: 0 - 7 are the sweep's, the heat baths', the tempered sweeps', the hops' and mcq_tabu's
constexpr int RHO_BITS = 15;              // rho_q < Q < 32^3 and rho_t < N^3 <= 32^3
constexpr int DELTA_BIAS = 13 * (MCQ_MAX_N_QUENCH3D - 1);  // 403: |delta| <= 13 (N - 1), so 0 <= delta + DELTA_BIAS <= 806 < 2^10
constexpr uint32_t RHO_MASK = (1u << RHO_BITS) - 1u;
constexpr uint32_t KEY_NONE = 0xFFFFFFFFu;                 // a cell key S << 15 | rho_t stays below 2^24 (S <= 13 (N - 1) + 1 = 404 < 2^9)
constexpr unsigned long long KEY64_NONE = ~0ull;           // a move key stays below 2^40
static_assert(MCQ_MAX_TABU3D_SPAN + REBASE + 1 < (1 << 16), "a stamp written just before the base moves fits 16 bits");

struct Tabu3dArgs {
    const uint32_t* seeds;
    const uint8_t* state_in;
    uint8_t* state_out;
    const uint16_t* tabu_in;
    uint16_t* tabu_out;
    const int32_t* best_floor;
    int32_t* energy_in;
    int32_t* energy_out;
    int32_t* best_energy;
    int64_t* best_iter;
    uint8_t* best_state;
    int64_t* n_moves;
    int64_t* n_aspired;
    int64_t* n_uphill;
    int64_t* n_stalled;
    int32_t* energy_hist;
    int32_t* flags;
    long long hist_stride;
    long long n_iters;
    long long first_iter;
    int tenure;
    int tenure_rand;
    int tenure_conf;
    int N;
    int Q;
};

// the per-chain figures, by one lane or by the host: `a` is the kernel's argument struct or the parameter block
template <class A>
__host__ __device__ __forceinline__ void store_tabu3d_figures(const A& a, long long ch, int e_in, int E, int B, long long best_iter, long long moves,
                                                              long long aspired, long long uphill, long long stalled, int flags) {
    if (a.energy_in) a.energy_in[ch] = e_in;
    if (a.energy_out) a.energy_out[ch] = E;
    if (a.best_energy) a.best_energy[ch] = B;
    if (a.best_iter) a.best_iter[ch] = best_iter;
    if (a.n_moves) a.n_moves[ch] = moves;
    if (a.n_aspired) a.n_aspired[ch] = aspired;
    if (a.n_uphill) a.n_uphill[ch] = uphill;
    if (a.n_stalled) a.n_stalled[ch] = stalled;
    if (a.flags) a.flags[ch] = flags;
}

// the words of iteration g: the two tie offsets and the tenure's jitter
__host__ __device__ __forceinline__ void tabu3d_draw(uint32_t seed, unsigned long long g, int Q, int C, int tenure_rand, int& oq, int& jitter, int& ot) {
    uint32_t r[4];
    philox_block((uint32_t)g, (uint32_t)(g >> 32), seed, TABU3D_KEY_WORD, r);
    oq = (int)(((unsigned long long)r[0] * (unsigned)Q) >> 32);
    jitter = (int)(((unsigned long long)r[1] * (unsigned)(tenure_rand + 1)) >> 32);
    ot = (int)(((unsigned long long)r[2] * (unsigned)C) >> 32);
}

// rule item 5
__host__ __device__ __forceinline__ int tabu3d_span(int tenure, int jitter, int tenure_conf, int F) {
    const int L = tenure + jitter + ((tenure_conf * F) >> 4);  // (64 (2^15 - 1) fits an int)
    return L < MCQ_MAX_TABU3D_SPAN ? L : MCQ_MAX_TABU3D_SPAN;
}

// the steps lo .. hi that keep x + step dc on the board
__host__ __device__ __forceinline__ void clip_steps(int dc, int x, int N, int& lo, int& hi) {
    if (dc > 0) lo = lo > -x ? lo : -x, hi = hi < N - 1 - x ? hi : N - 1 - x;
    if (dc < 0) lo = lo > x - (N - 1) ? lo : x - (N - 1), hi = hi < x ? hi : x;
}

// the minima of x and of y over the workgroup, through red[0 .. 15] and red[16 .. 31]
template <int W>
__device__ __forceinline__ void block_min2(uint32_t& x, uint32_t& y, uint32_t* red) {
    for (int o = 32; o; o >>= 1) {
        x = min(x, (uint32_t)__shfl_xor((int)x, o, 64));
        y = min(y, (uint32_t)__shfl_xor((int)y, o, 64));
    }
    if (W == 64) return;
    __syncthreads();  // the readers of the reduction before this one are done with red
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x, red[16 + (threadIdx.x >> 6)] = y;
    __syncthreads();
    x = red[0], y = red[16];
    for (int w = 1; w < W / 64; w++) x = min(x, red[w]), y = min(y, red[16 + w]);
}

// the minimum of a 64-bit key over the workgroup, through red as W / 64 pairs of dwords (all 32 at W = 1024)
template <int W>
__device__ __forceinline__ unsigned long long block_min64(unsigned long long v, uint32_t* red) {
    for (int o = 32; o; o >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o, 64);
        const unsigned long long other = (unsigned long long)hi << 32 | lo;
        v = other < v ? other : v;
    }
    if (W == 64) return v;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[2 * (threadIdx.x >> 6)] = (uint32_t)v, red[2 * (threadIdx.x >> 6) + 1] = (uint32_t)(v >> 32);
    __syncthreads();
    v = (unsigned long long)red[1] << 32 | red[0];
    for (int w = 1; w < W / 64; w++) {
        const unsigned long long other = (unsigned long long)red[2 * w + 1] << 32 | red[2 * w];
        v = other < v ? other : v;
    }
    return v;
}

template <int W, int BITS, int STEPS>
__global__ __launch_bounds__(W) void mcq_tabu3d_kernel(Tabu3dArgs a) {
    extern __shared__ uint32_t lds[];
    constexpr int CPD = 32 / BITS, SLOTS = 13 * STEPS;
    const int N = a.N, Q = a.Q, N2 = N * N, C = N2 * N;
    const int sw = (C + 1) / 2;  // dwords of stamps
    uint32_t* red = lds;
    uint32_t* const stamp32 = lds + 32;
    uint16_t* const stamp = reinterpret_cast<uint16_t*>(stamp32);
    const Chain chain = carve<BITS>(lds + 32 + sw, C);
    uint32_t* const field = chain.field;
    uint32_t* const occ = chain.occ;
    uint16_t* const queens = chain.queens;
    const int fw = chain.fw, bw = chain.bw;
    const int tid = threadIdx.x;
    const long long ch = blockIdx.x;
    const uint32_t seed = a.seeds[ch];
    const uint8_t* in = a.state_in + ch * 3 * Q;
    uint8_t* out = a.state_out + ch * 3 * Q;
    uint8_t* bs = a.best_state ? a.best_state + ch * 3 * Q : nullptr;
    int32_t* hist = a.energy_hist ? a.energy_hist + ch * a.hist_stride : nullptr;
    const uint16_t* ti = a.tabu_in ? a.tabu_in + ch * C : nullptr;
    uint16_t* to = a.tabu_out ? a.tabu_out + ch * C : nullptr;

    for (int w = tid; w < fw + bw; w += W) field[w] = 0;  // (field and occ are adjacent)
    for (int w = tid; w < sw; w += W) {                   // the stamps, relative to first_iter; the half behind an odd N^3 is 0
        uint32_t v = 0;
        if (ti) v = (uint32_t)ti[2 * w] | (2 * w + 1 < C ? (uint32_t)ti[2 * w + 1] << 16 : 0u);
        stamp32[w] = v;
    }
    __syncthreads();
    if (tid == 0) set_pad_bits(occ, bw, C);
    __syncthreads();
    int rep = 0;
    for (int q = tid; q < Q; q += W) rep |= load_queen(queens, occ, in, N, q);
    __syncthreads();  // queens, occ and the stamps are complete; every byte of state_in and tabu_in is read
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
        if (to)
            for (int c = tid; c < C; c += W) to[c] = stamp[c];
        if (tid == 0) store_tabu3d_figures(a, ch, e, e, e, 0, 0, 0, 0, 0, MCQ_TABU3D_REPEATED);
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
    long long moves = 0, aspired = 0, uphill = 0, stalled = 0, best_iter = 0;
    if (hist && tid == 0) hist[0] = E;

    long long t_base = 0;  // the iteration of the call at which the stamps' base lies
    for (long long t = 0; t < a.n_iters; t++) {
        if (t - t_base == REBASE) {  // (uniform: the arguments alone decide)
            __syncthreads();
            for (int w = tid; w < sw; w += W) stamp32[w] = rebase2(stamp32[w]);
            t_base = t;
            __syncthreads();
        }
        const int now_rel = (int)(t - t_base);  // g less the base: a stamp above it is tabu
        int oq, jitter, ot;
        tabu3d_draw(seed, (unsigned long long)(a.first_iter + t), Q, C, a.tenure_rand, oq, jitter, ot);

        // (1) the cube: the smallest free cell that is not tabu, and the smallest that is
        uint32_t gfree = KEY_NONE, gtabu = KEY_NONE;
        for (int w = tid; w < fw; w += W) {
            const uint32_t v = field[w];
            const int c0 = w * CPD;
            const uint32_t o = occ[c0 >> 5] >> (c0 & 31);
            // the stamps of the dword's cells, as dwords too: one at 16 bits per cell, two at 8 (the second may lie behind an odd end)
            const int s0 = c0 >> 1;
            const uint32_t st_lo = stamp32[s0], st_hi = CPD == 4 && s0 + 1 < sw ? stamp32[s0 + 1] : 0u;
#pragma unroll
            for (int b = 0; b < CPD; b++) {
                if ((o >> b) & 1u) continue;  // a queen, or a pad bit
                int rho = c0 + b - ot;
                rho += rho < 0 ? C : 0;
                const uint32_t key = ((v >> (b * BITS)) & ((1u << BITS) - 1u)) << RHO_BITS | (uint32_t)rho;
                const int st = (int)(((b < 2 ? st_lo : st_hi) >> (16 * (b & 1))) & 0xFFFFu);
                if (st > now_rel) gtabu = min(gtabu, key);
                else gfree = min(gfree, key);
            }
        }
        block_min2<W>(gfree, gtabu, red);

        // (2) the queens: each conflicting queen's best target, as the move's key
        const int room = B - E;  // <= 0: T_q = room + c
        unsigned long long best_key = KEY64_NONE;
        int f = 0;
        for (int q = tid; q < Q; q += W) {
            const int p = queens[q];
            const int pi = p >> 10, pj = (p >> 5) & 31, pk = p & 31;
            const int c = field_at<BITS>(field, (pi * N + pj) * N + pk) - 1;
            if (c <= 0) continue;
            f++;
            const int Tq = room + c;
            uint32_t key = gfree;
            if ((int)(gtabu >> RHO_BITS) < Tq) key = min(key, gtabu);  // (KEY_NONE >> 15 is above every T_q)
            for (int d = 0; d < 13; d++) {
                int di, dj, dk;
                direction(d, di, dj, dk);
                int lo = -(N - 1), hi = N - 1;
                clip_steps(di, pi, N, lo, hi), clip_steps(dj, pj, N, lo, hi), clip_steps(dk, pk, N, lo, hi);
                for (int step = lo; step <= hi; step++) {
                    const int cell = ((pi + step * di) * N + pj + step * dj) * N + pk + step * dk;
                    if ((occ[cell >> 5] >> (cell & 31)) & 1u) continue;  // (the queen's own cell, step 0, among them)
                    const int val = field_at<BITS>(field, cell) - 1;
                    if ((int)stamp[cell] > now_rel && !(val < Tq)) continue;
                    int rho = cell - ot;
                    rho += rho < 0 ? C : 0;
                    key = min(key, (uint32_t)val << RHO_BITS | (uint32_t)rho);
                }
            }
            if (key != KEY_NONE) {
                const int delta = (int)(key >> RHO_BITS) - c;
                int rq = q - oq;
                rq += rq < 0 ? Q : 0;
                const unsigned long long mk = (unsigned long long)(uint32_t)(delta + DELTA_BIAS) << (2 * RHO_BITS) | (unsigned long long)(uint32_t)rq << RHO_BITS | (key & RHO_MASK);
                best_key = mk < best_key ? mk : best_key;
            }
        }
        const int F = block_sum<W>(f, red);
        best_key = block_min64<W>(best_key, red);

        // (3), (4): the move, or none (uniform: best_key is the same in every lane)
        if (best_key == KEY64_NONE) {
            stalled++;
        } else {
            const int delta = (int)(best_key >> (2 * RHO_BITS)) - DELTA_BIAS;
            int q = (int)((best_key >> RHO_BITS) & RHO_MASK) + oq;
            q -= q >= Q ? Q : 0;
            int tcell = (int)(best_key & RHO_MASK) + ot;
            tcell -= tcell >= C ? C : 0;
            const int p = queens[q];
            const int pcell = cell_of(p, N);
            const int tp = packed_of(tcell, N, N2);
            aspired += (int)stamp[tcell] > now_rel;
            uphill += delta > 0;
            moves++;
            const int L = tabu3d_span(a.tenure, jitter, a.tenure_conf, F);
            __syncthreads();  // every lane has read queens[q] and the stamp, and both passes are over, before the queen moves
            put<W, BITS, STEPS>(field, N, p, -1, tid, W, SLOTS);
            put<W, BITS, STEPS>(field, N, tp, +1, tid, W, SLOTS);
            if (tid == 0) {
                vacate(occ, pcell);
                occupy(occ, queens, q, tp, tcell);
                stamp[pcell] = (uint16_t)(now_rel + 1 + L);
            }
            __syncthreads();
            E += delta;
            if (E < B) {
                B = E, best_iter = t + 1;
                if (bs) store_queens(bs, queens, Q, tid, W);
            }
        }
        if (hist && tid == 0) hist[t + 1] = E;
    }
    __syncthreads();

    store_queens(out, queens, Q, tid, W);
    if (to) {
        const int end_rel = (int)(a.n_iters - t_base);  // first_iter + n_iters less the base
        for (int c = tid; c < C; c += W) {
            const int st = stamp[c];
            to[c] = (uint16_t)(st > end_rel ? st - end_rel : 0);
        }
    }
    if (tid == 0) store_tabu3d_figures(a, ch, e_in, E, B, best_iter, moves, aspired, uphill, stalled, 0);
}

// the bytes of LDS of a chain: red, the stamps, the field, occ and the queens
long long lds_bytes(int N, int Q) {
    const long long cells = (long long)N * N * N, cpd = N <= 19 ? 4 : 2;
    return 4 * (32 + (cells + 1) / 2 + (cells + cpd - 1) / cpd + (cells + 31) / 32 + ((long long)Q + 1) / 2);
}

// what both entry points refuse
int check_tabu3d(const mcq_tabu3d* q) {
    if (!q) return fail(g_tabu3d_err, MCQ_EINVAL, "mcq_tabu3d: NULL parameter block");
    const int rc = mcq_post::check_full3d(g_tabu3d_err, "tabu search", q->N, q->n_queens, (long long)q->n_chains);
    if (rc != MCQ_OK) return rc;
    if (q->n_iters < 0) return fail(g_tabu3d_err, MCQ_EINVAL, "n_iters must be >= 0 (0 = the recount), got %lld", (long long)q->n_iters);
    if (q->first_iter < 0) return fail(g_tabu3d_err, MCQ_EINVAL, "first_iter must be >= 0, got %lld", (long long)q->first_iter);
    if ((unsigned long long)q->first_iter + (unsigned long long)q->n_iters >= (1ull << 63))
        return fail(g_tabu3d_err, MCQ_EINVAL, "iterations: first_iter + n_iters must stay below 2^63 (first_iter %lld, n_iters %lld)", (long long)q->first_iter,
                    (long long)q->n_iters);
    if (q->tenure < 0 || q->tenure > MCQ_MAX_TABU_TENURE)
        return fail(g_tabu3d_err, MCQ_EINVAL, "tenure out of range [0, %d]: %d", MCQ_MAX_TABU_TENURE, (int)q->tenure);
    if (q->tenure_rand < 0 || q->tenure_rand > MCQ_MAX_TABU_TENURE_RAND)
        return fail(g_tabu3d_err, MCQ_EINVAL, "tenure_rand out of range [0, %d]: %d", MCQ_MAX_TABU_TENURE_RAND, (int)q->tenure_rand);
    if (q->tenure_conf < 0 || q->tenure_conf > MCQ_MAX_TABU_TENURE_CONF)
        return fail(g_tabu3d_err, MCQ_EINVAL, "tenure_conf out of range [0, %d]: %d", MCQ_MAX_TABU_TENURE_CONF, (int)q->tenure_conf);
    if (!q->seeds) return fail(g_tabu3d_err, MCQ_EINVAL, "seeds is required");
    if (!q->state_in) return fail(g_tabu3d_err, MCQ_EINVAL, "state_in is required");
    if (!q->state_out) return fail(g_tabu3d_err, MCQ_EINVAL, "state_out is required");
    if (q->energy_hist && q->hist_stride < q->n_iters + 1)
        return fail(g_tabu3d_err, MCQ_EINVAL, "hist_stride must be >= n_iters + 1 = %lld, got %lld", (long long)q->n_iters + 1, (long long)q->hist_stride);
    if (q->best_state && (q->best_state == q->state_in || q->best_state == q->state_out))
        return fail(g_tabu3d_err, MCQ_EINVAL, "best_state must be distinct from state_in and state_out (it is written while they are in use)");
    return MCQ_OK;
}

// chains first .. last - 1 through the rule, with an int field per cell and absolute stamps
void host_chains(const mcq_tabu3d* q, long long first, long long last) {
    const int N = q->N, Q = queens_of(q);
    HostField f(N, Q);
    const std::vector<int>& S = f.S;
    const int C = f.C, N2 = f.N2;
    std::vector<long long> T((size_t)C);
    for (long long ch = first; ch < last; ch++) {
        const bool repeated = f.load(q->state_in + ch * 3 * Q);
        const int e_in = f.energy();
        uint8_t* bs = q->best_state ? q->best_state + ch * 3 * Q : nullptr;
        int32_t* hist = q->energy_hist ? q->energy_hist + ch * q->hist_stride : nullptr;
        const uint16_t* ti = q->tabu_in ? q->tabu_in + ch * C : nullptr;
        uint16_t* to = q->tabu_out ? q->tabu_out + ch * C : nullptr;
        if (bs) f.store(bs);
        if (repeated) {
            f.store(q->state_out + ch * 3 * Q);
            if (hist)
                for (long long t = 0; t <= q->n_iters; t++) hist[t] = e_in;
            if (to)
                for (int c = 0; c < C; c++) to[c] = ti ? ti[c] : (uint16_t)0;
            store_tabu3d_figures(*q, ch, e_in, e_in, e_in, 0, 0, 0, 0, 0, MCQ_TABU3D_REPEATED);
            continue;
        }
        for (int c = 0; c < C; c++) T[(size_t)c] = ti ? q->first_iter + (long long)ti[c] : 0LL;
        int E = e_in, B = e_in;
        if (q->best_floor && q->best_floor[ch] < B) B = q->best_floor[ch];
        long long moves = 0, aspired = 0, uphill = 0, stalled = 0, best_iter = 0;
        if (hist) hist[0] = E;
        const uint32_t seed = q->seeds[ch];
        for (long long t = 0; t < q->n_iters; t++) {
            const long long g = q->first_iter + t;
            int oq, jitter, ot;
            tabu3d_draw(seed, (unsigned long long)g, Q, C, q->tenure_rand, oq, jitter, ot);
            auto rho_of = [&](int cell) { return cell - ot + (cell < ot ? C : 0); };
            // the smallest (S, rho_t) over the free cells that are not tabu, and over those that are
            int fs = INT_MAX, fr = 0, ts = INT_MAX, tr = 0;
            for (int c = 0; c < C; c++) {
                if (f.occ[(size_t)c]) continue;
                const int s = S[(size_t)c], r = rho_of(c);
                if (T[(size_t)c] > g) {
                    if (s < ts || (s == ts && r < tr)) ts = s, tr = r;
                } else if (s < fs || (s == fs && r < fr)) {
                    fs = s, fr = r;
                }
            }
            int F = 0, bd = INT_MAX, brq = 0, brt = 0;
            for (int n = 0; n < Q; n++) {
                const int p = f.pos[(size_t)n], c = S[(size_t)p] - 1;
                if (c <= 0) continue;
                F++;
                const int Tq = B - E + c;  // a tabu target is admissible when its a(n, t) is below this
                int v = fs, r = fr;        // this queen's smallest (a(n, t), rho_t); INT_MAX: none
                if (ts < Tq && (ts < v || (ts == v && tr < r))) v = ts, r = tr;
                const int pi = p / N2, pj = (p / N) % N, pk = p % N;
                for (int d = 0; d < 13; d++) {  // the cells on its lines count the queen itself
                    int di, dj, dk;
                    direction(d, di, dj, dk);
                    int lo = -(N - 1), hi = N - 1;
                    clip_steps(di, pi, N, lo, hi), clip_steps(dj, pj, N, lo, hi), clip_steps(dk, pk, N, lo, hi);
                    for (int step = lo; step <= hi; step++) {
                        const int cell = ((pi + step * di) * N + pj + step * dj) * N + pk + step * dk;
                        if (f.occ[(size_t)cell]) continue;
                        const int val = S[(size_t)cell] - 1, rr = rho_of(cell);
                        if (T[(size_t)cell] > g && !(val < Tq)) continue;
                        if (val < v || (val == v && rr < r)) v = val, r = rr;
                    }
                }
                if (v == INT_MAX) continue;
                const int delta = v - c, rq = n - oq + (n < oq ? Q : 0);
                if (delta < bd || (delta == bd && (rq < brq || (rq == brq && r < brt)))) bd = delta, brq = rq, brt = r;
            }
            if (bd == INT_MAX) {
                stalled++;
            } else {
                const int n = (brq + oq) % Q, cell = (brt + ot) % C, p = f.pos[(size_t)n];
                aspired += T[(size_t)cell] > g;
                uphill += bd > 0;
                moves++;
                T[(size_t)p] = g + 1 + tabu3d_span(q->tenure, jitter, q->tenure_conf, F);
                f.take_out(n);
                f.put_back(n, cell);
                E += bd;
                if (E < B) {
                    B = E, best_iter = t + 1;
                    if (bs) f.store(bs);
                }
            }
            if (hist) hist[t + 1] = E;
        }
        f.store(q->state_out + ch * 3 * Q);
        if (to) {
            const long long end = q->first_iter + q->n_iters;
            for (int c = 0; c < C; c++) to[c] = (uint16_t)(T[(size_t)c] > end ? T[(size_t)c] - end : 0);
        }
        store_tabu3d_figures(*q, ch, e_in, E, B, best_iter, moves, aspired, uphill, stalled, 0);
    }
}

}  // namespace

extern "C" {

const char* mcq_tabu3d_last_error(void) { return g_tabu3d_err; }

int mcq_tabu3d_host(const mcq_tabu3d* q) {
    const int rc = check_tabu3d(q);
    if (rc != MCQ_OK) return rc;
    mcq_post::for_chains((long long)q->n_chains, [q](long long first, long long last) { host_chains(q, first, last); });
    return MCQ_OK;
}

int mcq_tabu3d_device(const mcq_tabu3d* q, void* hip_stream) {
    const int rc = check_tabu3d(q);
    if (rc != MCQ_OK) return rc;
    const int Q = queens_of(q);
    const long long bytes = lds_bytes(q->N, Q);
    if (bytes > MCQ_MAX_TABU3D_LDS)
        return fail(g_tabu3d_err, MCQ_EINVAL, "N = %d with n_queens = %d: a chain takes %lld bytes of LDS, above the %d of a workgroup "
                    "(mcq_tabu3d_device runs every Q = N^2; mcq_tabu3d_host runs every shape)", (int)q->N, Q, bytes, MCQ_MAX_TABU3D_LDS);
    hipStream_t s = (hipStream_t)hip_stream;
    const Tabu3dArgs a{q->seeds, q->state_in, q->state_out, q->tabu_in, q->tabu_out, q->best_floor, q->energy_in, q->energy_out, q->best_energy,
                       q->best_iter, q->best_state, q->n_moves, q->n_aspired, q->n_uphill, q->n_stalled, q->energy_hist, q->flags,
                       (long long)q->hist_stride, (long long)q->n_iters, (long long)q->first_iter, (int)q->tenure, (int)q->tenure_rand,
                       (int)q->tenure_conf, (int)q->N, Q};
    const int cells = a.N * a.N * a.N;
    const hipError_t e = for_shape_of(a.N, [&](auto shape) {
        using S = decltype(shape);
        return launch<S>(mcq_tabu3d_kernel<S::W, S::BITS, S::STEPS>, a, a.N, a.Q, 32 + (cells + 1) / 2, (long long)q->n_chains, s);
    });
    if (e != hipSuccess) return fail(g_tabu3d_err, MCQ_EDEVICE, "mcq_tabu3d_device: %s", hipGetErrorString(e));
    return MCQ_OK;
}

}  // extern "C"
