// mcq_heatbath3d.hip -- heat-bath queen sweeps of full_3d placements (include/mcq.h: mcq_heatbath3d, where the rule is stated).  Like the
// quench of full_3d placements (csrc/mcq_quench3d.hip) it sits outside the Metropolis sweep and lives on the ATTACK FIELD S(t) = the number
// of queens that hold or attack cell t: with queen q taken out, S(t) IS a(q, t) for every cell, so one pass over the field gives the whole
// Boltzmann distribution of the queen over its N^3 - Q + 1 targets.
//
//   kernel  one chain per workgroup of W lanes (64, 256 or 1024), the quench's three instantiations and its layout, all in dynamic LDS:
//             red     32 dwords            the cross-wavefront half of the minimum
//             scan    16 x uint64          the wavefront totals of the prefix sum
//             win     2 dwords (+ pad)     the selected cell and its count
//             tab     512 dwords           the sweep's table row, staged once per sweep
//             field / occ / queens         as in the quench: 8- or 16-bit counts read as whole dwords, the occupancy bitmap with its
//                                          pad bits set, Q packed cells i << 10 | j << 5 | k
//           (137 504 bytes at N = 32, Q = N^3 - 1).  Taking a queen out and putting it back is the quench's `put`: one 32-bit LDS atomic
//           per cell of the 13 lines.  Per queen update, between the two:
//             1. the minimum of S over the free cells: per lane, then __shfl_xor, then red;
//             2. the weights.  Cell-index order is part of the rule, so lane l owns the CONTIGUOUS run of R field dwords from l R on,
//                R = ceil(dwords / W) rounded up to an ODD number: ds_read_b32 banks by dword index mod 32 over each half of the
//                wavefront, and an odd stride sends the 32 lanes of a half to 32 different banks.  R <= 17 dwords = 34 cells at N = 32
//                and 7 dwords = 28 cells at N <= 19, so a lane's own sum stays below 2^30; the prefix over lanes is 64-bit: DPP row
//                shifts inside a row of 16 lanes, the four row totals by v_readlane, the wavefront totals through `scan`;
//             3. U = __umul64hi(x, W), and the ONE lane whose interval [P, P + sum) holds U walks its run again and writes the winner
//                to `win`.  Everything after that barrier is uniform over the workgroup, so every barrier is reached by all lanes;
//             4. one Philox block per two queens, the same counter in every lane (the compiler keeps it on the scalar unit).
//           A REPEATED placement breaks the byte bound of the field and is never put into it: pairwise recount, written back unmoved.
//           At N <= 4 (at most 16 field dwords) most of the 64 lanes idle; several chains per wavefront are out of scope.
//   host    mcq_heatbath3d_host: the same rule with an int field per cell, a plain scan and 128-bit arithmetic for U.
//
// Built for gfx950 only, with csrc/mcq_hip.hip:  hipcc --offload-arch=gfx950 -O3 -ffp-contract=off
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdarg>
#include <cstdio>
#include <thread>
#include <vector>

#include "../../include/mcq.h"

namespace {

thread_local char g_heatbath3d_err[256] = "";

int heatbath3d_fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_heatbath3d_err, sizeof g_heatbath3d_err, fmt, ap);
    va_end(ap);
    return code;
}

// philox4x32-10: counter (c0, c1, 0, 0), key (k0, k1)
__host__ __device__ __forceinline__ void philox_block(uint32_t c0, uint32_t c1, uint32_t k0, uint32_t k1, uint32_t out[4]) {
    uint32_t c2 = 0, c3 = 0;
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1, c3 = (uint32_t)p0, c0 = n0, c2 = n2;
        k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
    }
    out[0] = c0, out[1] = c1, out[2] = c2, out[3] = c3;
}

struct Heatbath3dArgs {
    const uint32_t* seeds;
    const uint32_t* table;
    const uint8_t* state_in;
    uint8_t* state_out;
    int32_t* energy_in;
    int32_t* energy_out;
    int32_t* best_energy;
    int64_t* best_sweep;
    uint8_t* best_state;
    int64_t* n_changed;
    int32_t* energy_hist;
    int32_t* flags;
    long long hist_stride;
    long long n_sweeps;
    long long first_sweep;
    int table_len;
    int N;
    int Q;
};

constexpr int HDR = 72;    // dwords of red, scan and win
constexpr int TAB = MCQ_MAX_HEATBATH_TABLE;

// direction d = 0 .. 12: the half of {-1, 0, 1}^3 \ {0} whose first non-zero component is +1, as the digits of d + 14 in base 3
__host__ __device__ __forceinline__ void direction(int d, int& di, int& dj, int& dk) {
    const int c = d + 14;
    di = c / 9 - 1, dj = (c / 3) % 3 - 1, dk = c % 3 - 1;
}

// the non-zero ones among |di|, |dj|, |dk| are all equal (the same cell included: a shared cell counts as an attacking pair)
__host__ __device__ __forceinline__ bool attacks(int pa, int pb) {
    const int di = abs((pa >> 10) - (pb >> 10)), dj = abs(((pa >> 5) & 31) - ((pb >> 5) & 31)), dk = abs((pa & 31) - (pb & 31));
    const int m = max(di, max(dj, dk));
    return (di == 0 || di == m) && (dj == 0 || dj == m) && (dk == 0 || dk == m);
}

// (no barrier in front: between the readers of one queen's minimum and the writers of the next lie the barriers of the update)
template <int W>
__device__ __forceinline__ uint32_t block_min(uint32_t v, uint32_t* red) {
    for (int o = 32; o; o >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, o, 64));
    if (W == 64) return v;
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    v = red[0];
    for (int w = 1; w < W / 64; w++) v = min(v, red[w]);
    return v;
}

template <int W>
__device__ __forceinline__ int block_sum(int v, uint32_t* red) {
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o, 64);
    if (W == 64) return v;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = (uint32_t)v;
    __syncthreads();
    v = (int)red[0];
    for (int w = 1; w < W / 64; w++) v += (int)red[w];
    return v;
}

// DPP within a row of 16 lanes: the value of the lane `n` below, 0 where the row ends
template <int n>
__device__ __forceinline__ unsigned long long row_shr64(unsigned long long v) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)v, 0x110 + n, 0xF, 0xF, false);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(v >> 32), 0x110 + n, 0xF, 0xF, false);
    return (unsigned long long)hi << 32 | lo;
}

template <int lane>
__device__ __forceinline__ unsigned long long read_lane64(unsigned long long v) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, lane), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), lane);
    return (unsigned long long)hi << 32 | lo;
}

// EXCLUSIVE prefix sum of `own` over the lanes of the workgroup in lane order; `total` = the workgroup's sum
template <int W>
__device__ __forceinline__ unsigned long long block_scan(uint32_t own, unsigned long long* scan, unsigned long long& total) {
    unsigned long long v = own;
    v += row_shr64<1>(v);
    v += row_shr64<2>(v);
    v += row_shr64<4>(v);
    v += row_shr64<8>(v);
    const unsigned long long r0 = read_lane64<15>(v), r1 = read_lane64<31>(v), r2 = read_lane64<47>(v), r3 = read_lane64<63>(v);
    const int lane = threadIdx.x & 63;
    v += (lane >= 16 ? r0 : 0ull) + (lane >= 32 ? r1 : 0ull) + (lane >= 48 ? r2 : 0ull);
    total = r0 + r1 + r2 + r3;
    v -= own;
    if (W == 64) return v;
    const int wave = threadIdx.x >> 6;
    if (lane == 0) scan[wave] = total;
    __syncthreads();
    unsigned long long before = 0, all = 0;
    for (int w = 0; w < W / 64; w++) {
        const unsigned long long t = scan[w];
        before += w < wave ? t : 0ull;
        all += t;
    }
    total = all;
    return v + before;
}

// S(cell) of a field of BITS-wide entries
template <int BITS>
__device__ __forceinline__ int field_at(const uint32_t* field, int cell) {
    constexpr int CPD = 32 / BITS;  // cells per dword
    return (int)((field[cell / CPD] >> ((cell % CPD) * BITS)) & ((1u << BITS) - 1u));
}

// S += sign on the cell p (packed) and on every in-bounds cell of the 13 lines through it: this lane's slots of queen p
template <int W, int BITS, int STEPS>
__device__ __forceinline__ void put(uint32_t* field, int N, int p, int sign, int first_slot, int stride, int n_slots) {
    constexpr int CPD = 32 / BITS;
    const int pi = p >> 10, pj = (p >> 5) & 31, pk = p & 31;
    for (int s = first_slot; s < n_slots; s += stride) {
        const int d = s / STEPS, step = (s % STEPS) - (N - 1);  // step = -(N - 1) .. N - 1 where s % STEPS <= 2 N - 2
        int di, dj, dk;
        direction(d, di, dj, dk);
        const int i = pi + step * di, j = pj + step * dj, k = pk + step * dk;
        const bool on = step < N && (step != 0 || d == 0) && (unsigned)i < (unsigned)N && (unsigned)j < (unsigned)N && (unsigned)k < (unsigned)N;
        if (on) {
            const int cell = (i * N + j) * N + k;
            const uint32_t one = 1u << ((cell % CPD) * BITS);
            atomicAdd(&field[cell / CPD], sign > 0 ? one : 0u - one);
        }
    }
}

__device__ __forceinline__ void store_queens(uint8_t* out, const uint16_t* queens, int Q, int tid, int W) {
    for (int q = tid; q < Q; q += W) {
        const int p = queens[q];
        out[3 * q] = (uint8_t)(p >> 10), out[3 * q + 1] = (uint8_t)((p >> 5) & 31), out[3 * q + 2] = (uint8_t)(p & 31);
    }
}

template <int W, int BITS, int STEPS>
__global__ __launch_bounds__(W) void mcq_heatbath3d_kernel(Heatbath3dArgs a) {
    extern __shared__ uint32_t lds[];
    constexpr int CPD = 32 / BITS, SLOTS = 13 * STEPS;
    constexpr uint32_t MASK = (1u << BITS) - 1u;
    const int N = a.N, Q = a.Q, N2 = N * N, C = N2 * N, D = a.table_len;
    const int fw = (C + CPD - 1) / CPD, bw = (C + 31) / 32;
    uint32_t* red = lds;
    unsigned long long* scan = (unsigned long long*)(lds + 32);
    uint32_t* win = lds + 64;
    uint32_t* tab = lds + HDR;
    uint32_t* field = tab + TAB;
    uint32_t* occ = field + fw;
    uint16_t* queens = (uint16_t*)(occ + bw);
    const int tid = threadIdx.x;
    const long long ch = blockIdx.x;
    const uint8_t* in = a.state_in + ch * 3 * Q;
    uint8_t* out = a.state_out + ch * 3 * Q;
    uint8_t* bout = a.best_state ? a.best_state + ch * 3 * Q : nullptr;
    int32_t* hist = a.energy_hist ? a.energy_hist + ch * a.hist_stride : nullptr;

    for (int w = tid; w < fw + bw; w += W) field[w] = 0;  // (field and occ are adjacent)
    __syncthreads();
    if (tid == 0) {
        if (C & 31) occ[bw - 1] = ~0u << (C & 31);  // the pad bits: never a candidate
        win[0] = win[1] = 0;
    }
    __syncthreads();
    int rep = 0;
    for (int q = tid; q < Q; q += W) {
        const int i = min((int)in[3 * q], N - 1), j = min((int)in[3 * q + 1], N - 1), k = min((int)in[3 * q + 2], N - 1);
        queens[q] = (uint16_t)(i << 10 | j << 5 | k);
        const int cell = (i * N + j) * N + k;
        const uint32_t bit = 1u << (cell & 31);
        rep |= (atomicOr(&occ[cell >> 5], bit) & bit) != 0;
    }
    const bool repeated = __syncthreads_or(rep) != 0;  // (a barrier: queens and occ are complete, every byte of state_in is read)
    store_queens(out, queens, Q, tid, W);  // the clamped input: what n_sweeps = 0 and a repeated placement hand back
    if (bout) store_queens(bout, queens, Q, tid, W);

    if (repeated) {
        int twoE = 0;
        for (int q = tid; q < Q; q += W) {
            const int p = queens[q];
            int n = 0;
            for (int o = 0; o < Q; o++) n += attacks(p, queens[o]);
            twoE += n - 1;  // itself
        }
        const int e = block_sum<W>(twoE, red) >> 1;
        if (hist)
            for (long long s = tid; s <= a.n_sweeps; s += W) hist[s] = e;
        if (tid == 0) {
            if (a.energy_in) a.energy_in[ch] = e;
            if (a.energy_out) a.energy_out[ch] = e;
            if (a.best_energy) a.best_energy[ch] = e;
            if (a.best_sweep) a.best_sweep[ch] = 0;
            if (a.n_changed) a.n_changed[ch] = 0;
            if (a.flags) a.flags[ch] = MCQ_HEATBATH3D_REPEATED;
        }
        return;
    }

    // the field of all queens: every (queen, slot) pair is one atomic add
    for (int x = tid; x < Q * SLOTS; x += W) put<W, BITS, STEPS>(field, N, queens[x / SLOTS], +1, x % SLOTS, SLOTS, SLOTS);
    __syncthreads();
    int twoE = 0;
    for (int q = tid; q < Q; q += W) {
        const int p = queens[q];
        twoE += field_at<BITS>(field, ((p >> 10) * N + ((p >> 5) & 31)) * N + (p & 31)) - 1;
    }
    const int e_in = block_sum<W>(twoE, red) >> 1;
    if (hist && tid == 0) hist[0] = e_in;

    // this lane's run of field dwords: R is odd, so the lanes of an access group read 32 different banks
    const int R = ((fw + W - 1) / W) | 1;
    const int w0 = min(tid * R, fw), w1 = min(w0 + R, fw);
    const uint32_t seed = a.seeds[ch];
    int E = e_in, best = e_in;
    long long best_sweep = 0, changed = 0;
    uint32_t rnd[4] = {0, 0, 0, 0};
    for (long long s = 0; s < a.n_sweeps; s++) {
        const uint32_t* row = a.table + s * D;
        for (int d = tid; d < D; d += W) tab[d] = row[d];  // (its readers of the sweep before are behind that sweep's last barrier)
        const unsigned long long u0 = (unsigned long long)(a.first_sweep + s) * (unsigned long long)Q;
        for (int q = 0; q < Q; q++) {
            const int p = queens[q];
            const int pcell = ((p >> 10) * N + ((p >> 5) & 31)) * N + (p & 31);
            put<W, BITS, STEPS>(field, N, p, -1, tid, W, SLOTS);
            if (tid == 0) occ[pcell >> 5] &= ~(1u << (pcell & 31));
            __syncthreads();  // the field is a(q, .), the table row is staged
            const int a_old = field_at<BITS>(field, pcell);
            uint32_t m = ~0u;
            for (int w = w0; w < w1; w++) {
                const uint32_t v = field[w];
                const uint32_t o = occ[(w * CPD) >> 5] >> ((w * CPD) & 31);
#pragma unroll
                for (int b = 0; b < CPD; b++)
                    if (!((o >> b) & 1u)) m = min(m, (v >> (b * BITS)) & MASK);
            }
            const int a_min = (int)block_min<W>(m, red);
            uint32_t own = 0;
            for (int w = w0; w < w1; w++) {
                const uint32_t v = field[w];
                const uint32_t o = occ[(w * CPD) >> 5] >> ((w * CPD) & 31);
#pragma unroll
                for (int b = 0; b < CPD; b++)
                    if (!((o >> b) & 1u)) own += tab[min((int)((v >> (b * BITS)) & MASK) - a_min, D - 1)];
            }
            unsigned long long Wt;
            const unsigned long long before = block_scan<W>(own, scan, Wt);
            const unsigned long long u = u0 + (unsigned)q;
            if ((u & 1) == 0 || q == 0) philox_block((uint32_t)(u >> 1), (uint32_t)(u >> 33), seed, 2u, rnd);
            const unsigned long long x = (u & 1) ? ((unsigned long long)rnd[3] << 32 | rnd[2]) : ((unsigned long long)rnd[1] << 32 | rnd[0]);
            const unsigned long long U = __umul64hi(x, Wt);
            if (own != 0 && before <= U && U < before + own) {  // one lane, as U < W: walk the run again to the smallest t with C_t > U
                unsigned long long c = before;
                bool found = false;
                for (int w = w0; w < w1 && !found; w++) {
                    const uint32_t v = field[w];
                    const uint32_t o = occ[(w * CPD) >> 5] >> ((w * CPD) & 31);
#pragma unroll
                    for (int b = 0; b < CPD; b++)
                        if (!found && !((o >> b) & 1u)) {
                            const int cnt = (int)((v >> (b * BITS)) & MASK);
                            c += tab[min(cnt - a_min, D - 1)];
                            if (c > U) {
                                win[0] = (uint32_t)(w * CPD + b), win[1] = (uint32_t)cnt;
                                found = true;
                            }
                        }
                }
            }
            __syncthreads();  // win is written; every lane has read queens[q] and the whole field before the queen goes back
            int t = p, tcell = pcell, a_new = a_old;
            if (Wt != 0) {  // (uniform.  W = 0: only a table with T[0] = 0; the queen stays)
                tcell = (int)win[0], a_new = (int)win[1];
                const int ti = tcell / N2, tj = (tcell - ti * N2) / N;
                t = ti << 10 | tj << 5 | (tcell - ti * N2 - tj * N);
            }
            E += a_new - a_old;
            changed += tcell != pcell;
            put<W, BITS, STEPS>(field, N, t, +1, tid, W, SLOTS);
            if (tid == 0) {
                occ[tcell >> 5] |= 1u << (tcell & 31);
                queens[q] = (uint16_t)t;
            }
            __syncthreads();
        }
        if (hist && tid == 0) hist[s + 1] = E;
        if (E < best) {
            best = E;
            best_sweep = s + 1;
            if (bout) store_queens(bout, queens, Q, tid, W);
        }
    }

    if (a.n_sweeps > 0) store_queens(out, queens, Q, tid, W);
    if (tid == 0) {
        if (a.energy_in) a.energy_in[ch] = e_in;
        if (a.energy_out) a.energy_out[ch] = E;
        if (a.best_energy) a.best_energy[ch] = best;
        if (a.best_sweep) a.best_sweep[ch] = best_sweep;
        if (a.n_changed) a.n_changed[ch] = changed;
        if (a.flags) a.flags[ch] = 0;
    }
}

int queens_of(const mcq_heatbath3d* q) { return q->n_queens == 0 ? q->N * q->N : q->n_queens; }

// what both entry points refuse
int check_heatbath3d(const mcq_heatbath3d* q) {
    if (!q) return heatbath3d_fail(MCQ_EINVAL, "mcq_heatbath3d: NULL parameter block");
    if (q->N > MCQ_MAX_N_QUENCH3D && q->N <= MCQ_MAX_N)
        return heatbath3d_fail(MCQ_EINVAL, "N out of range [%d, %d]: %d (the full_3d heat-bath sweep stops at N = %d, where a cell index fits 15 bits; the sweep runs to %d)",
                               MCQ_MIN_N, MCQ_MAX_N_QUENCH3D, (int)q->N, MCQ_MAX_N_QUENCH3D, MCQ_MAX_N);
    if (q->N < MCQ_MIN_N || q->N > MCQ_MAX_N_QUENCH3D) return heatbath3d_fail(MCQ_EINVAL, "N out of range [%d, %d]: %d", MCQ_MIN_N, MCQ_MAX_N_QUENCH3D, (int)q->N);
    const int cells = q->N * q->N * q->N;
    if (q->n_queens != 0 && (q->n_queens < 2 || q->n_queens > cells - 1))
        return heatbath3d_fail(MCQ_EINVAL, "n_queens out of range [2, N^3 - 1 = %d] (0 = N^2): %d", cells - 1, (int)q->n_queens);
    if (q->n_chains < 1 || q->n_chains > INT_MAX) return heatbath3d_fail(MCQ_EINVAL, "n_chains out of range [1, 2^31 - 1]: %lld", (long long)q->n_chains);
    if (q->n_sweeps < 0) return heatbath3d_fail(MCQ_EINVAL, "n_sweeps must be >= 0, got %lld", (long long)q->n_sweeps);
    if (q->first_sweep < 0) return heatbath3d_fail(MCQ_EINVAL, "first_sweep must be >= 0, got %lld", (long long)q->first_sweep);
    const uint64_t end = (uint64_t)q->first_sweep + (uint64_t)q->n_sweeps, Q = (uint64_t)queens_of(q);
    if (end > ((1ull << 62) - 1) / Q)
        return heatbath3d_fail(MCQ_EINVAL, "first_sweep + n_sweeps = %llu: the update index (first_sweep + n_sweeps) Q must stay below 2^62", (unsigned long long)end);
    if (q->table_len < 1 || q->table_len > MCQ_MAX_HEATBATH_TABLE)
        return heatbath3d_fail(MCQ_EINVAL, "table_len out of range [1, %d]: %lld", MCQ_MAX_HEATBATH_TABLE, (long long)q->table_len);
    if (!q->seeds) return heatbath3d_fail(MCQ_EINVAL, "seeds is required");
    if (!q->table && q->n_sweeps > 0) return heatbath3d_fail(MCQ_EINVAL, "table is required (n_sweeps rows of table_len words)");
    if (!q->state_in) return heatbath3d_fail(MCQ_EINVAL, "state_in is required");
    if (!q->state_out) return heatbath3d_fail(MCQ_EINVAL, "state_out is required");
    if (q->energy_hist && q->hist_stride < q->n_sweeps + 1)
        return heatbath3d_fail(MCQ_EINVAL, "hist_stride must be >= n_sweeps + 1 = %lld, got %lld", (long long)q->n_sweeps + 1, (long long)q->hist_stride);
    return MCQ_OK;
}

template <int W, int BITS, int STEPS>
hipError_t launch_heatbath3d(const Heatbath3dArgs& a, long long n_chains, hipStream_t s) {
    const int cells = a.N * a.N * a.N, cpd = 32 / BITS;
    const size_t bytes = 4 * (size_t)(HDR + TAB + (cells + cpd - 1) / cpd + (cells + 31) / 32 + (a.Q + 1) / 2);
    if (bytes > 32 * 1024) {  // (the default limit is 64 KiB with the kernel's static LDS; a chain at N = 32 takes up to 135 KiB)
        const hipError_t e = hipFuncSetAttribute((const void*)mcq_heatbath3d_kernel<W, BITS, STEPS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((mcq_heatbath3d_kernel<W, BITS, STEPS>), dim3((unsigned)n_chains), dim3(W), bytes, s, a);
    return hipGetLastError();
}

// chains first .. last - 1 through the rule, with an int field per cell
void host_chains(const mcq_heatbath3d* q, long long first, long long last) {
    const int N = q->N, Q = queens_of(q), N2 = N * N, C = N2 * N, D = (int)q->table_len;
    std::vector<int> S((size_t)C), pos((size_t)Q);
    std::vector<uint8_t> occ((size_t)C);
    // S += sign on the cell and on the 13 lines through it
    auto put = [&](int cell, int sign) {
        const int pi = cell / N2, pj = (cell / N) % N, pk = cell % N;
        S[(size_t)cell] += sign;
        for (int d = 0; d < 13; d++) {
            int di, dj, dk;
            direction(d, di, dj, dk);
            for (int step = -(N - 1); step < N; step++) {
                const int i = pi + step * di, j = pj + step * dj, k = pk + step * dk;
                if (step != 0 && i >= 0 && i < N && j >= 0 && j < N && k >= 0 && k < N) S[(size_t)((i * N + j) * N + k)] += sign;
            }
        }
    };
    auto store = [&](uint8_t* out) {
        for (int n = 0; n < Q; n++) {
            const int p = pos[(size_t)n];
            out[3 * n] = (uint8_t)(p / N2), out[3 * n + 1] = (uint8_t)((p / N) % N), out[3 * n + 2] = (uint8_t)(p % N);
        }
    };
    for (long long ch = first; ch < last; ch++) {
        const uint8_t* in = q->state_in + ch * 3 * Q;
        uint8_t* bout = q->best_state ? q->best_state + ch * 3 * Q : nullptr;
        int32_t* hist = q->energy_hist ? q->energy_hist + ch * q->hist_stride : nullptr;
        for (int c = 0; c < C; c++) S[(size_t)c] = 0, occ[(size_t)c] = 0;
        bool repeated = false;
        for (int n = 0; n < Q; n++) {
            const int i = in[3 * n] < N ? in[3 * n] : N - 1, j = in[3 * n + 1] < N ? in[3 * n + 1] : N - 1, k = in[3 * n + 2] < N ? in[3 * n + 2] : N - 1;
            const int cell = (i * N + j) * N + k;
            pos[(size_t)n] = cell;
            repeated |= occ[(size_t)cell] != 0;
            occ[(size_t)cell] = 1;
            put(cell, +1);
        }
        long long twoE = 0;
        for (int n = 0; n < Q; n++) twoE += S[(size_t)pos[(size_t)n]] - 1;
        const int e_in = (int)(twoE / 2);
        int E = e_in, best = e_in;
        long long best_sweep = 0, changed = 0;
        if (hist) hist[0] = e_in;
        if (bout) store(bout);
        const uint32_t seed = q->seeds[ch];
        for (long long s = 0; s < q->n_sweeps; s++) {
            if (repeated) {
                if (hist) hist[s + 1] = e_in;
                continue;
            }
            const uint32_t* T = q->table + s * D;
            const uint64_t u0 = (uint64_t)(q->first_sweep + s) * (uint64_t)Q;
            for (int n = 0; n < Q; n++) {
                const int p = pos[(size_t)n];
                put(p, -1);
                occ[(size_t)p] = 0;
                int a_min = INT_MAX;
                for (int c = 0; c < C; c++)
                    if (!occ[(size_t)c] && S[(size_t)c] < a_min) a_min = S[(size_t)c];
                uint64_t Wt = 0;
                for (int c = 0; c < C; c++)
                    if (!occ[(size_t)c]) Wt += T[std::min(S[(size_t)c] - a_min, D - 1)];
                const uint64_t u = u0 + (uint64_t)n;
                uint32_t r[4];
                philox_block((uint32_t)(u >> 1), (uint32_t)(u >> 33), seed, 2u, r);
                const uint64_t x = (u & 1) ? ((uint64_t)r[3] << 32 | r[2]) : ((uint64_t)r[1] << 32 | r[0]);
                const uint64_t U = (uint64_t)(((unsigned __int128)x * Wt) >> 64);
                int t = p;
                if (Wt != 0) {
                    uint64_t c_sum = 0;
                    for (int c = 0; c < C; c++) {
                        if (occ[(size_t)c]) continue;
                        c_sum += T[std::min(S[(size_t)c] - a_min, D - 1)];
                        if (c_sum > U) {
                            t = c;
                            break;
                        }
                    }
                }
                E += S[(size_t)t] - S[(size_t)p];
                changed += t != p;
                put(t, +1);
                occ[(size_t)t] = 1;
                pos[(size_t)n] = t;
            }
            if (hist) hist[s + 1] = E;
            if (E < best) {
                best = E;
                best_sweep = s + 1;
                if (bout) store(bout);
            }
        }
        store(q->state_out + ch * 3 * Q);
        if (q->energy_in) q->energy_in[ch] = e_in;
        if (q->energy_out) q->energy_out[ch] = E;
        if (q->best_energy) q->best_energy[ch] = best;
        if (q->best_sweep) q->best_sweep[ch] = best_sweep;
        if (q->n_changed) q->n_changed[ch] = changed;
        if (q->flags) q->flags[ch] = repeated ? MCQ_HEATBATH3D_REPEATED : 0;
    }
}

}  // namespace

extern "C" {

const char* mcq_heatbath3d_last_error(void) { return g_heatbath3d_err; }

int mcq_heatbath3d_host(const mcq_heatbath3d* q) {
    const int rc = check_heatbath3d(q);
    if (rc != MCQ_OK) return rc;
    // chains do not interact: a few threads share them
    const long long n = q->n_chains;
    const unsigned hw = std::thread::hardware_concurrency();
    const long long n_threads = std::min<long long>(std::min<long long>(hw ? hw : 1, 16), (n + 63) / 64);
    if (n_threads <= 1) {
        host_chains(q, 0, n);
    } else {
        std::vector<std::thread> pool;
        for (long long t = 0; t < n_threads; t++) pool.emplace_back(host_chains, q, n * t / n_threads, n * (t + 1) / n_threads);
        for (auto& t : pool) t.join();
    }
    return MCQ_OK;
}

int mcq_heatbath3d_device(const mcq_heatbath3d* q, void* hip_stream) {
    const int rc = check_heatbath3d(q);
    if (rc != MCQ_OK) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    const Heatbath3dArgs a{q->seeds, q->table, q->state_in, q->state_out, q->energy_in, q->energy_out, q->best_energy, q->best_sweep, q->best_state,
                           q->n_changed, q->energy_hist, q->flags, (long long)q->hist_stride, (long long)q->n_sweeps, (long long)q->first_sweep,
                           (int)q->table_len, (int)q->N, queens_of(q)};
    // the quench's instantiation table: lanes per chain, field width, steps per direction of an update (2 N - 1 <= STEPS)
    hipError_t e;
    if (q->N <= 12) e = launch_heatbath3d<64, 8, 32>(a, (long long)q->n_chains, s);
    else if (q->N <= 19) e = launch_heatbath3d<256, 8, 64>(a, (long long)q->n_chains, s);
    else e = launch_heatbath3d<1024, 16, 64>(a, (long long)q->n_chains, s);
    if (e != hipSuccess) return heatbath3d_fail(MCQ_EDEVICE, "mcq_heatbath3d_device: %s", hipGetErrorString(e));
    return MCQ_OK;
}

}  // extern "C"
