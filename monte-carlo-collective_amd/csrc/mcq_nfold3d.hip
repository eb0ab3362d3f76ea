// mcq_nfold3d.hip -- the n-fold way of Bortz, Kalos and Lebowitz for full_3d placements: the Metropolis dynamics of the reference's
// default move (a uniform queen to a uniform cell that holds no queen) without its rejections (include/mcq.h: mcq_nfold3d, where the rule
// is stated).  The field, `put`, `carve`, the shapes and `launch` are those of csrc/mcq_field.h; the clock and `clock_ell` are
// restated from csrc/mcq_nfold.hip, the line walk from csrc/mcq_tabu3d.hip and the weighted draw over the cube from
// csrc/mcq_heatbath3d.hip, which keep theirs in anonymous namespaces.
//
//   kernel  one chain per workgroup of W lanes (64, 256 or 1024), all in dynamic LDS:
//             red     32 dwords            the cross-wavefront half of a minimum
//             scan    16 x uint64          the wavefront totals of a prefix sum
//             win     8 dwords             the drawn queen, what is left of U behind it, the drawn cell and its d
//             T       512 dwords           the segment's weight row
//             clk     256 dwords           the clock table
//             H       512 dwords           H[f] = the number of free cells with S = f
//             G       512 x uint64         G[c] = sum over f of H[f] T[clamp(f - c)]: R(q) of a queen with c_q = c that attacked nothing
//             R       Q x uint64           R(q)
//             field / occ / queens         csrc/mcq_field.h; the field is that of the WHOLE placement, built once per launch
//           Nobody walks Q N^3 pairs.  For a free cell t, a(q, t) = S(t) - [pos(q) attacks t], so R(q) = G(c_q) + corr(q), corr(q) the
//           sum over the <= 13 (N - 1) free cells on q's own lines of T[clamp(S - 1 - c_q)] - T[clamp(S - c_q)] (uint64, wrapping; the
//           sum is exact).  EVENT: (1) H is recounted by a pass over the cube, with its largest f; (2) G, a lane per c; (3) R(q), a
//           contiguous run of queens per lane, and a 64-bit scan over the lanes gives W; (4) the clock, in every lane alike; (5) the ONE
//           lane whose run holds U walks it for q; (6) a pass over the cube in cell order, a contiguous run of field dwords per lane as
//           in the heat bath, gives w(q, t), a second scan, and the one lane whose run holds the rest of U walks it for t; (7) two
//           `put`s, and best_state goes to global memory when the best falls.  H, G and every R are formed again behind every event.
//           Every branch around a barrier is taken on values that every lane computed alike from the arguments, the scans' totals or
//           `win` behind a barrier, so every barrier is reached by all lanes.
//   host    mcq_nfold3d_host: the DEFINITION on HostField, every (q, t) pair with plain loops and unsigned __int128, for every shape.
//           It shares nothing of the decomposition above.
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
using mcq_post::philox_block;
using mcq_post::queens_of;

typedef unsigned long long u64;

thread_local char g_nfold3d_err[256] = "";

constexpr uint32_t NFOLD3D_KEY_WORD = 12u;  // key word 1 of the chain's Philox stream: 0 - 11 are taken (include/mcq.h: mcq_nfold3d, item 4)
constexpr int TB = MCQ_NFOLD_TIME_BITS;
constexpr int TAB = MCQ_MAX_NFOLD3D_TABLE;
constexpr int HIST = 512;  // entries of H and G: S of a free cell and c_q are at most 13 (N - 1) = 403
constexpr int HDR = 72;    // dwords of red, scan and win
constexpr int EXTRA = HDR + TAB + 256 + HIST + 2 * HIST;  // dwords in front of R; even, so that G and R are 8-byte aligned
constexpr uint32_t NONE = 0xFFFFFFFFu;
static_assert(13 * (MCQ_MAX_N_QUENCH3D - 1) + 1 < HIST && 13 * (MCQ_MAX_N_QUENCH3D - 1) < TAB, "H, G and the row hold every count");
static_assert(EXTRA % 2 == 0, "uint64 arrays behind the dwords");

struct Nfold3dArgs {
    const uint32_t* seeds;
    const uint32_t* table;
    const uint32_t* clock_table;
    const uint64_t* need_in;
    const int64_t* events_in;
    const uint8_t* state_in;
    uint8_t* state_out;
    uint8_t* best_state;
    int32_t* energy_in;
    int32_t* energy_out;
    int32_t* best_energy;
    int64_t* best_step;
    int64_t* events_out;
    int64_t* n_uphill;
    int64_t* n_flat;
    uint64_t* need_out;
    uint64_t* weight_out;
    int32_t* energy_hist;
    int32_t* flags;
    long long hist_stride;
    long long n_segs;
    long long seg_steps;
    uint32_t clock_ln2;
    int table_len;
    int N;
    int Q;
};

// the per-chain figures, by one lane or by the host: `a` is the kernel's argument struct or the parameter block
template <class A>
__host__ __device__ __forceinline__ void store_nfold3d_figures(const A& a, long long ch, int e_in, int E, int best_e, long long best_step, u64 events,
                                                               long long up, long long flat, u64 need, u64 W, int flags) {
    if (a.energy_in) a.energy_in[ch] = e_in;
    if (a.energy_out) a.energy_out[ch] = E;
    if (a.best_energy) a.best_energy[ch] = best_e;
    if (a.best_step) a.best_step[ch] = best_step;
    if (a.events_out) a.events_out[ch] = (int64_t)events;
    if (a.n_uphill) a.n_uphill[ch] = up;
    if (a.n_flat) a.n_flat[ch] = flat;
    if (a.need_out) a.need_out[ch] = need;
    if (a.weight_out) a.weight_out[ch] = W;
    if (a.flags) a.flags[ch] = flags;
}

// l(x) of the board rule's item 5: z clock_ln2 + clock_table[y], z the leading zero bits of x and y the 8 bits below its leading one bit
__host__ __device__ __forceinline__ uint32_t clock_ell(uint32_t x, uint32_t ln2, const uint32_t* clock_table) {
    const int z = x ? __builtin_clz(x) : 32;
    const uint32_t y = x ? ((x << z) >> 23) & 255u : 0u;
    return (uint32_t)z * ln2 + clock_table[y];
}

// T[min(max(d, 0), D - 1)]
__host__ __device__ __forceinline__ uint32_t weight_of(const uint32_t* T, int d, int last) { return T[d < 0 ? 0 : d > last ? last : d]; }

// the steps lo .. hi that keep x + step dc on the board
__host__ __device__ __forceinline__ void clip_steps(int dc, int x, int N, int& lo, int& hi) {
    if (dc > 0) lo = lo > -x ? lo : -x, hi = hi < N - 1 - x ? hi : N - 1 - x;
    if (dc < 0) lo = lo > x - (N - 1) ? lo : x - (N - 1), hi = hi < x ? hi : x;
}

// rule item 3 in 64-bit arithmetic: whether the event fires within `left`, and its tau
__device__ __forceinline__ bool event_fires(u64 need, u64 W, u64 left, u64& tau) {
    const u64 q1 = need / W;
    if (q1 >> 32) return false;  // tau >= 2^44 > left
    const u64 r1 = need - q1 * W;  // r1 < W < 2^52
    tau = (q1 << TB) + ((r1 << TB) / W);
    tau = tau ? tau : 1ull;
    return tau <= left;
}

// floor(left W / 2^12) of the 96-bit product; the quotient is at most need < 2^58
__device__ __forceinline__ u64 hazard_spent(u64 left, u64 W) { return (__umul64hi(left, W) << (64 - TB)) | ((left * W) >> TB); }

// EXCLUSIVE prefix sum of `own` over the lanes of the workgroup in lane order; `total` = the workgroup's sum
template <int W>
__device__ __forceinline__ u64 block_scan(u64 own, u64* scan, u64& total) {
    const int lane = threadIdx.x & 63;
    u64 incl = own;
    for (int o = 1; o < 64; o <<= 1) {
        const u64 t = __shfl_up(incl, o, 64);
        incl += lane >= o ? t : 0ull;
    }
    total = __shfl(incl, 63, 64);
    const u64 v = incl - own;
    if (W == 64) return v;
    const int wave = threadIdx.x >> 6;
    if (lane == 0) scan[wave] = total;
    __syncthreads();
    u64 before = 0, all = 0;
    for (int w = 0; w < W / 64; w++) {
        const u64 t = scan[w];
        before += w < wave ? t : 0ull;
        all += t;
    }
    total = all;
    return v + before;
}

template <int W, int BITS, int STEPS>
__global__ __launch_bounds__(W) void mcq_nfold3d_kernel(Nfold3dArgs a) {
    extern __shared__ uint32_t lds[];
    constexpr int CPD = 32 / BITS, SLOTS = 13 * STEPS;
    constexpr uint32_t MASK = (1u << BITS) - 1u;
    const int N = a.N, Q = a.Q, N2 = N * N, C = N2 * N, D = a.table_len, last = D - 1;
    uint32_t* red = lds;
    u64* scan = (u64*)(lds + 32);
    uint32_t* win = lds + 64;
    uint32_t* T = lds + HDR;
    uint32_t* clk = T + TAB;
    uint32_t* H = clk + 256;
    u64* G = (u64*)(H + HIST);
    u64* Rq = G + HIST;
    const auto [field, occ, queens, fw, bw] = carve<BITS>((uint32_t*)(Rq + Q), C);
    const int tid = threadIdx.x;
    const long long ch = blockIdx.x;
    const uint32_t seed = a.seeds[ch];
    const uint8_t* in = a.state_in + ch * 3 * Q;
    uint8_t* out = a.state_out + ch * 3 * Q;
    uint8_t* bs = a.best_state ? a.best_state + ch * 3 * Q : nullptr;
    int32_t* hist = a.energy_hist ? a.energy_hist + ch * a.hist_stride : nullptr;

    for (int w = tid; w < fw + bw; w += W) field[w] = 0;  // (field and occ are adjacent)
    for (int i = tid; i < 256; i += W) clk[i] = a.clock_table[i];
    __syncthreads();
    if (tid == 0) set_pad_bits(occ, bw, C);
    __syncthreads();
    int rep = 0;
    for (int q = tid; q < Q; q += W) rep |= load_queen(queens, occ, in, N, q);
    __syncthreads();  // queens, occ and clk are complete; every byte of state_in is read
    const bool repeated = block_sum<W>(rep, red) != 0;
    store_queens(out, queens, Q, tid, W);  // the clamped input: what n_segs = 0 and a repeated placement hand back
    if (bs) store_queens(bs, queens, Q, tid, W);

    u64 e = a.events_in ? (u64)a.events_in[ch] : 0ull;
    uint32_t x[4];
    philox_block((uint32_t)e, (uint32_t)(e >> 32), seed, NFOLD3D_KEY_WORD, x);
    const u64 M = (u64)Q * (u64)(C - Q);
    u64 need = a.need_in ? a.need_in[ch] : M * clock_ell(x[2], a.clock_ln2, clk);

    if (repeated) {  // rule item 1: recounted pair by pair, handed back unmoved
        int twoE = 0;
        for (int q = tid; q < Q; q += W) {
            const int p = queens[q];
            int n = 0;
            for (int o = 0; o < Q; o++) n += attacks(p, queens[o]);
            twoE += n - 1;  // itself
        }
        const int er = block_sum<W>(twoE, red) >> 1;
        if (hist)
            for (long long s = tid; s <= a.n_segs; s += W) hist[s] = er;
        if (tid == 0) store_nfold3d_figures(a, ch, er, er, er, 0, e, 0, 0, need, 0ull, MCQ_NFOLD3D_REPEATED);
        return;
    }

    for (int i = tid; i < Q * SLOTS; i += W) put_slot<W, BITS, STEPS>(field, queens, N, i);
    __syncthreads();
    int twoE = 0;
    for (int q = tid; q < Q; q += W) twoE += attackers_at<BITS>(field, N, queens[q]);
    const int e_in = block_sum<W>(twoE, red) >> 1;

    int E = e_in, best_e = e_in;
    long long best_step = 0, up = 0, flat = 0;
    u64 Wt = 0;
    if (hist && tid == 0) hist[0] = E;

    const int fcap = 13 * (N - 1);  // the largest S of a free cell, and the largest c_q
    // this lane's run of field dwords (odd, so that the lanes of an access group read different banks) and its run of queens
    const int RW = ((fw + W - 1) / W) | 1;
    const int w0 = min(tid * RW, fw), w1 = min(w0 + RW, fw);
    const int QC = (Q + W - 1) / W;
    const int q0 = min(tid * QC, Q), q1 = min(q0 + QC, Q);

    for (long long s = 0; s < a.n_segs; s++) {
        __syncthreads();  // the row of the segment before has been read
        for (int i = tid; i < D; i += W) T[i] = a.table[s * D + i];
        const u64 whole = (u64)a.seg_steps << TB;
        u64 left = whole;
        for (;;) {
            // (1) H and its largest f
            for (int f = tid; f <= fcap; f += W) H[f] = 0;
            if (tid == 0) win[0] = NONE;
            __syncthreads();  // (also: the row is staged; the field, occ and queens of the event before are complete)
            uint32_t fm = 0;
            for (int w = tid; w < fw; w += W) {
                const uint32_t v = field[w];
                const uint32_t o = occ[(w * CPD) >> 5] >> ((w * CPD) & 31);
#pragma unroll
                for (int b = 0; b < CPD; b++)
                    if (!((o >> b) & 1u)) {  // neither a queen nor a pad bit
                        const uint32_t f = min((v >> (b * BITS)) & MASK, (uint32_t)(HIST - 1));  // (S <= 13 (N - 1): the bound only keeps a broken field inside H)
                        atomicAdd(&H[f], 1u);
                        fm = max(fm, f);
                    }
            }
            const int fmax = (int)~block_min<W, true>(~fm, red);
            __syncthreads();  // H is complete
            // (2) G, a lane per c
            for (int c = tid; c <= fcap; c += W) {
                u64 g = 0;
                for (int f = 0; f <= fmax; f++) g += (u64)H[f] * weight_of(T, f - c, last);
                G[c] = g;
            }
            __syncthreads();
            // (3) R(q) = G(c_q) + corr(q) over this lane's queens, and W
            u64 own = 0;
            for (int q = q0; q < q1; q++) {
                const int p = queens[q];
                const int pi = p >> 10, pj = (p >> 5) & 31, pk = p & 31;
                const int c = field_at<BITS>(field, (pi * N + pj) * N + pk) - 1;
                u64 r = G[min(max(c, 0), HIST - 1)];  // (0 <= c <= 13 (N - 1))
                for (int d = 0; d < 13; d++) {
                    int di, dj, dk;
                    direction(d, di, dj, dk);
                    int lo = -(N - 1), hi = N - 1;
                    clip_steps(di, pi, N, lo, hi), clip_steps(dj, pj, N, lo, hi), clip_steps(dk, pk, N, lo, hi);
                    for (int step = lo; step <= hi; step++) {
                        const int cell = ((pi + step * di) * N + pj + step * dj) * N + pk + step * dk;
                        if ((occ[cell >> 5] >> (cell & 31)) & 1u) continue;  // (the queen's own cell, step 0, among them)
                        const int dd = field_at<BITS>(field, cell) - c;
                        r += (u64)weight_of(T, dd - 1, last) - (u64)weight_of(T, dd, last);
                    }
                }
                Rq[q] = r;
                own += r;
            }
            const u64 before = block_scan<W>(own, scan, Wt);
            // (4) the clock: every lane holds the same W, need and left
            if (Wt == 0) break;  // nothing can move under this row: the chain sleeps
            u64 tau = 0;
            if (!event_fires(need, Wt, left, tau)) {
                need -= hazard_spent(left, Wt);
                break;
            }
            left -= tau;
            // (5) the queen: the first q whose inclusive prefix of R exceeds U
            const u64 U = __umul64hi(((u64)x[0] << 32) | x[1], Wt);
            if (own != 0 && before <= U && U - before < own) {  // one lane, as U < W
                u64 u = U - before;
                for (int q = q0; q < q1; q++) {
                    const u64 r = Rq[q];
                    if (u < r) {
                        win[0] = (uint32_t)q, win[1] = (uint32_t)u, win[2] = (uint32_t)(u >> 32);
                        break;
                    }
                    u -= r;
                }
            }
            if (tid == 0) win[3] = NONE;
            __syncthreads();
            const int q = (int)win[0];
            if (win[0] == NONE) break;  // (cannot happen -- U < W --: it only ends a broken rule)
            const u64 u = (u64)win[2] << 32 | win[1];
            const int p = queens[q];
            const int pcell = cell_of(p, N);
            const int c = field_at<BITS>(field, pcell) - 1;
            // (6) the cell: the first free t in cell order whose inclusive prefix of w(q, t) exceeds what is left of U
            u64 ownc = 0;
            for (int w = w0; w < w1; w++) {
                const uint32_t v = field[w];
                const uint32_t o = occ[(w * CPD) >> 5] >> ((w * CPD) & 31);
#pragma unroll
                for (int b = 0; b < CPD; b++)
                    if (!((o >> b) & 1u)) {
                        const int at = (int)((v >> (b * BITS)) & MASK) - (int)attacks(p, packed_of(w * CPD + b, N, N2));
                        ownc += weight_of(T, at - c, last);
                    }
            }
            u64 Rt;
            const u64 beforec = block_scan<W>(ownc, scan, Rt);
            if (ownc != 0 && beforec <= u && u - beforec < ownc) {  // one lane, as u < R(q)
                u64 pre = beforec;
                bool found = false;
                for (int w = w0; w < w1 && !found; w++) {
                    const uint32_t v = field[w];
                    const uint32_t o = occ[(w * CPD) >> 5] >> ((w * CPD) & 31);
#pragma unroll
                    for (int b = 0; b < CPD; b++)
                        if (!found && !((o >> b) & 1u)) {
                            const int at = (int)((v >> (b * BITS)) & MASK) - (int)attacks(p, packed_of(w * CPD + b, N, N2));
                            pre += weight_of(T, at - c, last);
                            if (pre > u) {
                                win[3] = (uint32_t)(w * CPD + b), win[4] = (uint32_t)(at - c);
                                found = true;
                            }
                        }
                }
            }
            __syncthreads();  // win is written; every lane has read queens[q] and the whole field before the queen moves
            if (win[3] == NONE) break;  // (cannot happen -- the cells' weights sum to R(q) --: it only ends a broken rule)
            const int tcell = (int)win[3], dd = (int)win[4];
            const int tp = packed_of(tcell, N, N2);
            // (7) the move
            put<W, BITS, STEPS>(field, N, p, -1, tid, W, SLOTS);
            put<W, BITS, STEPS>(field, N, tp, +1, tid, W, SLOTS);
            if (tid == 0) {
                vacate(occ, pcell);
                occupy(occ, queens, q, tp, tcell);
            }
            __syncthreads();
            E += dd, up += dd > 0, flat += dd == 0, e++;
            if (E < best_e) {
                best_e = E, best_step = s * a.seg_steps + (long long)((whole - left) >> TB);
                if (bs) store_queens(bs, queens, Q, tid, W);
            }
            philox_block((uint32_t)e, (uint32_t)(e >> 32), seed, NFOLD3D_KEY_WORD, x);
            need = M * clock_ell(x[2], a.clock_ln2, clk);
        }
        if (hist && tid == 0) hist[s + 1] = E;
    }
    __syncthreads();

    if (a.n_segs > 0) store_queens(out, queens, Q, tid, W);
    if (tid == 0) store_nfold3d_figures(a, ch, e_in, E, best_e, best_step, e, up, flat, need, Wt, 0);
}

// the bytes of LDS of a chain: the dwords in front, R, the field, occ and the queens
long long lds_bytes(int N, int Q) {
    const long long cells = (long long)N * N * N, cpd = N <= 19 ? 4 : 2;
    return 4 * (EXTRA + 2 * (long long)Q + (cells + cpd - 1) / cpd + (cells + 31) / 32 + ((long long)Q + 1) / 2);
}

constexpr long long STEP_LIMIT = 1ll << MCQ_NFOLD_STEP_BITS;

// what both entry points refuse
int check_nfold3d(const mcq_nfold3d* q) {
    if (!q) return fail(g_nfold3d_err, MCQ_EINVAL, "mcq_nfold3d: NULL parameter block");
    if (q->mode != MCQ_MODE_FULL3D)
        return fail(g_nfold3d_err, MCQ_EINVAL, "mode: mcq_nfold3d runs full_3d placements only (MCQ_MODE_FULL3D; boards are mcq_nfold's), got %d", (int)q->mode);
    const int rc = mcq_post::check_full3d(g_nfold3d_err, "n-fold way", q->N, q->n_queens, (long long)q->n_chains);
    if (rc != MCQ_OK) return rc;
    if (q->n_segs < 0) return fail(g_nfold3d_err, MCQ_EINVAL, "n_segs must be >= 0, got %lld", (long long)q->n_segs);
    if (q->first_seg < 0) return fail(g_nfold3d_err, MCQ_EINVAL, "first_seg must be >= 0, got %lld", (long long)q->first_seg);
    if (q->seg_steps < 1 || q->seg_steps > (1ll << 31)) return fail(g_nfold3d_err, MCQ_EINVAL, "seg_steps out of range [1, 2^31]: %lld", (long long)q->seg_steps);
    if (q->n_segs >= STEP_LIMIT || q->first_seg >= STEP_LIMIT || q->first_seg + q->n_segs > (STEP_LIMIT - 1) / q->seg_steps)
        return fail(g_nfold3d_err, MCQ_EINVAL, "(first_seg + n_segs) seg_steps must stay below 2^%d: (%lld + %lld) * %lld", MCQ_NFOLD_STEP_BITS,
                    (long long)q->first_seg, (long long)q->n_segs, (long long)q->seg_steps);
    if (q->table_len < 1 || q->table_len > MCQ_MAX_NFOLD3D_TABLE)
        return fail(g_nfold3d_err, MCQ_EINVAL, "table_len out of range [1, %d]: %lld", MCQ_MAX_NFOLD3D_TABLE, (long long)q->table_len);
    if (q->clock_ln2 < 0 || q->clock_ln2 > (1ll << MCQ_NFOLD_WEIGHT_BITS))
        return fail(g_nfold3d_err, MCQ_EINVAL, "clock_ln2 out of range [0, 2^%d]: %lld", MCQ_NFOLD_WEIGHT_BITS, (long long)q->clock_ln2);
    if (!q->seeds) return fail(g_nfold3d_err, MCQ_EINVAL, "seeds is required");
    if (!q->state_in) return fail(g_nfold3d_err, MCQ_EINVAL, "state_in is required");
    if (!q->state_out) return fail(g_nfold3d_err, MCQ_EINVAL, "state_out is required");
    if (!q->clock_table) return fail(g_nfold3d_err, MCQ_EINVAL, "clock_table is required");
    if (!q->table && q->n_segs > 0) return fail(g_nfold3d_err, MCQ_EINVAL, "table is required when n_segs > 0");
    if (q->best_state && (q->best_state == q->state_in || q->best_state == q->state_out))
        return fail(g_nfold3d_err, MCQ_EINVAL, "best_state must be distinct from state_in and state_out (it is written while they are in use)");
    if (q->energy_hist && q->hist_stride < q->n_segs + 1)
        return fail(g_nfold3d_err, MCQ_EINVAL, "hist_stride must be >= n_segs + 1 = %lld, got %lld", (long long)q->n_segs + 1, (long long)q->hist_stride);
    return MCQ_OK;
}

// what the host entry can also look at: the entries of the tables and of the carried values
int check_nfold3d_entries(const mcq_nfold3d* q) {
    const long long D = q->table_len;
    for (long long i = 0; i < q->n_segs * D; i++)
        if (q->table[i] > (1u << MCQ_NFOLD_WEIGHT_BITS))
            return fail(g_nfold3d_err, MCQ_EINVAL, "table[%lld][%lld] = %u exceeds 2^%d", i / D, i % D, q->table[i], MCQ_NFOLD_WEIGHT_BITS);
    for (int i = 0; i < 256; i++)
        if (q->clock_table[i] > (1u << MCQ_NFOLD_CLOCK_BITS))
            return fail(g_nfold3d_err, MCQ_EINVAL, "clock_table[%d] = %u exceeds 2^%d", i, q->clock_table[i], MCQ_NFOLD_CLOCK_BITS);
    for (long long ch = 0; ch < q->n_chains; ch++) {
        if (q->need_in && q->need_in[ch] >= (1ull << MCQ_NFOLD3D_NEED_BITS))
            return fail(g_nfold3d_err, MCQ_EINVAL, "need_in[%lld] = %llu is not below 2^%d", ch, (unsigned long long)q->need_in[ch], MCQ_NFOLD3D_NEED_BITS);
        if (q->events_in && q->events_in[ch] < 0) return fail(g_nfold3d_err, MCQ_EINVAL, "events_in[%lld] must be >= 0, got %lld", ch, (long long)q->events_in[ch]);
    }
    return MCQ_OK;
}

// chains first .. last - 1 through the DEFINITION: every (q, t) pair behind every event, 128-bit arithmetic for the clock and U.  The cells
// that hold no queen are listed in cell order behind every event (their index, S and coordinates), so that the loop over t is a plain
// loop over that list
void host_chains(const mcq_nfold3d* q, long long first, long long last_chain) {
    typedef unsigned __int128 u128;
    const int N = q->N, Q = queens_of(q), last = (int)q->table_len - 1;
    HostField f(N, Q);
    const std::vector<int>& S = f.S;
    const int C = f.C, N2 = f.N2, F = C - Q;
    std::vector<int> ft((size_t)F), fS((size_t)F), fi((size_t)F), fj((size_t)F), fk((size_t)F);
    std::vector<u64> Rv((size_t)Q);
    const uint32_t ln2 = (uint32_t)q->clock_ln2;
    const u64 M = (u64)Q * (u64)F;
    // d of queen (pi, pj, pk) with c_q = c and free cell x: a(q, t) = S(t) - [p attacks t], the non-zero ones among |di|, |dj|, |dk| all equal
    const int *const pS = fS.data(), *const pI = fi.data(), *const pJ = fj.data(), *const pK = fk.data();
    auto diff = [=](int pi, int pj, int pk, int c, int x) {
        const int di = abs(pI[x] - pi), dj = abs(pJ[x] - pj), dk = abs(pK[x] - pk);
        const int m = di > dj ? (di > dk ? di : dk) : (dj > dk ? dj : dk);
        const int hit = ((di == 0) | (di == m)) & ((dj == 0) | (dj == m)) & ((dk == 0) | (dk == m));
        return pS[x] - hit - c;
    };
    constexpr int BLOCK = 512;
    int at[BLOCK];
    for (long long ch = first; ch < last_chain; ch++) {
        const bool repeated = f.load(q->state_in + ch * 3 * Q);
        const int e_in = f.energy();
        uint8_t* bs = q->best_state ? q->best_state + ch * 3 * Q : nullptr;
        int32_t* hist = q->energy_hist ? q->energy_hist + ch * q->hist_stride : nullptr;
        if (bs) f.store(bs);
        const uint32_t seed = q->seeds[ch];
        u64 e = q->events_in ? (u64)q->events_in[ch] : 0ull;
        uint32_t x[4];
        philox_block((uint32_t)e, (uint32_t)(e >> 32), seed, NFOLD3D_KEY_WORD, x);
        u64 need = q->need_in ? q->need_in[ch] : M * clock_ell(x[2], ln2, q->clock_table);
        if (repeated) {
            f.store(q->state_out + ch * 3 * Q);
            if (hist)
                for (long long s = 0; s <= q->n_segs; s++) hist[s] = e_in;
            store_nfold3d_figures(*q, ch, e_in, e_in, e_in, 0, e, 0, 0, need, 0ull, MCQ_NFOLD3D_REPEATED);
            continue;
        }
        int E = e_in, best_e = e_in;
        long long best_step = 0, up = 0, flat = 0;
        u64 W = 0;
        if (hist) hist[0] = E;
        for (long long s = 0; s < q->n_segs; s++) {
            const uint32_t* T = q->table + s * q->table_len;
            const u64 whole = (u64)q->seg_steps << TB;
            u64 left = whole;
            for (;;) {
                for (int t = 0, n = 0; t < C; t++)
                    if (!f.occ[(size_t)t]) ft[(size_t)n] = t, fS[(size_t)n] = S[(size_t)t], fi[(size_t)n] = t / N2, fj[(size_t)n] = (t / N) % N, fk[(size_t)n++] = t % N;
                W = 0;
                for (int n = 0; n < Q; n++) {
                    const int p = f.pos[(size_t)n], c = S[(size_t)p] - 1, pi = p / N2, pj = (p / N) % N, pk = p % N;
                    u64 r = 0;
                    for (int t0 = 0; t0 < F; t0 += BLOCK) {  // (in blocks: the differences first, then the row's entries)
                        const int nb = F - t0 < BLOCK ? F - t0 : BLOCK;
                        for (int i = 0; i < nb; i++) {
                            const int d = diff(pi, pj, pk, c, t0 + i);
                            at[i] = d < 0 ? 0 : d > last ? last : d;
                        }
                        for (int i = 0; i < nb; i++) r += T[at[i]];
                    }
                    Rv[(size_t)n] = r;
                    W += r;
                }
                if (W == 0) break;
                const u128 t0 = ((u128)need << TB) / W;
                const u128 tau = t0 ? t0 : (u128)1;
                if (tau > (u128)left) {
                    need -= (u64)(((u128)left * W) >> TB);
                    break;
                }
                left -= (u64)tau;
                const u64 U = (u64)(((u128)(((u64)x[0] << 32) | x[1]) * W) >> 64);
                u64 prefix = 0;
                int n = 0;
                while (prefix + Rv[(size_t)n] <= U) prefix += Rv[(size_t)n++];  // (U < W: the walk ends among the queens)
                const int p = f.pos[(size_t)n], c = S[(size_t)p] - 1, pi = p / N2, pj = (p / N) % N, pk = p % N;
                int t = 0, dd = 0;
                for (;; t++) {  // (U - prefix < R(n): the walk ends inside the list)
                    dd = diff(pi, pj, pk, c, t);
                    prefix += weight_of(T, dd, last);
                    if (prefix > U) break;
                }
                f.take_out(n);
                f.put_back(n, ft[(size_t)t]);
                E += dd, up += dd > 0, flat += dd == 0, e++;
                if (E < best_e) {
                    best_e = E, best_step = s * q->seg_steps + (long long)((whole - left) >> TB);
                    if (bs) f.store(bs);
                }
                philox_block((uint32_t)e, (uint32_t)(e >> 32), seed, NFOLD3D_KEY_WORD, x);
                need = M * clock_ell(x[2], ln2, q->clock_table);
            }
            if (hist) hist[s + 1] = E;
        }
        f.store(q->state_out + ch * 3 * Q);
        store_nfold3d_figures(*q, ch, e_in, E, best_e, best_step, e, up, flat, need, q->n_segs > 0 ? W : 0ull, 0);
    }
}

// fn(first, last) over the chains: as mcq_post::for_chains, but a thread per chain (up to 16) once a chain's pairs are many -- an
// event of a large cube walks Q (N^3 - Q) of them
template <class F>
void for_heavy_chains(long long n, long long pairs, F fn) {
    const unsigned hw = std::thread::hardware_concurrency();
    const long long n_threads = std::min<long long>(std::min<long long>(hw ? hw : 1, 16), n);
    if (pairs < (1 << 20) || n_threads <= 1) return mcq_post::for_chains(n, fn);
    std::vector<std::thread> pool;
    for (long long t = 0; t < n_threads; t++) pool.emplace_back(fn, n * t / n_threads, n * (t + 1) / n_threads);
    for (auto& t : pool) t.join();
}

}  // namespace

extern "C" {

const char* mcq_nfold3d_last_error(void) { return g_nfold3d_err; }

int mcq_nfold3d_host(const mcq_nfold3d* q) {
    int rc = check_nfold3d(q);
    if (rc == MCQ_OK) rc = check_nfold3d_entries(q);
    if (rc != MCQ_OK) return rc;
    const long long Q = queens_of(q), cells = (long long)q->N * q->N * q->N;
    for_heavy_chains((long long)q->n_chains, Q * (cells - Q), [q](long long first, long long last) { host_chains(q, first, last); });
    return MCQ_OK;
}

int mcq_nfold3d_device(const mcq_nfold3d* q, void* hip_stream) {
    const int rc = check_nfold3d(q);
    if (rc != MCQ_OK) return rc;
    const int Q = queens_of(q);
    const long long bytes = lds_bytes(q->N, Q);
    if (bytes > MCQ_MAX_NFOLD3D_LDS)
        return fail(g_nfold3d_err, MCQ_EINVAL, "N = %d with n_queens = %d: a chain takes %lld bytes of LDS, above the %d of a workgroup "
                    "(mcq_nfold3d_device runs every Q = N^2; mcq_nfold3d_host runs every shape)", (int)q->N, Q, bytes, MCQ_MAX_NFOLD3D_LDS);
    hipStream_t s = (hipStream_t)hip_stream;
    const Nfold3dArgs a{q->seeds, q->table, q->clock_table, q->need_in, q->events_in, q->state_in, q->state_out, q->best_state, q->energy_in,
                        q->energy_out, q->best_energy, q->best_step, q->events_out, q->n_uphill, q->n_flat, q->need_out, q->weight_out,
                        q->energy_hist, q->flags, (long long)q->hist_stride, (long long)q->n_segs, (long long)q->seg_steps, (uint32_t)q->clock_ln2,
                        (int)q->table_len, (int)q->N, Q};
    const hipError_t e = for_shape_of(a.N, [&](auto shape) {
        using S = decltype(shape);
        return launch<S>(mcq_nfold3d_kernel<S::W, S::BITS, S::STEPS>, a, a.N, a.Q, EXTRA + 2 * a.Q, (long long)q->n_chains, s);
    });
    if (e != hipSuccess) return fail(g_nfold3d_err, MCQ_EDEVICE, "mcq_nfold3d_device: %s", hipGetErrorString(e));
    return MCQ_OK;
}

}  // extern "C"
