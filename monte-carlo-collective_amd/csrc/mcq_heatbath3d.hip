// mcq_heatbath3d.hip -- heat-bath queen sweeps of full_3d placements (include/mcq.h: mcq_heatbath3d, where the rule is stated).  Like the
// quench of full_3d placements (csrc/mcq_quench3d.hip) it sits outside the Metropolis sweep and lives on the ATTACK FIELD S(t) = the number
// of queens that hold or attack cell t: with queen q taken out, S(t) IS a(q, t) for every cell, so one pass over the field gives the whole
// Boltzmann distribution of the queen over its N^3 - Q + 1 targets.
//
//   kernel  one chain per workgroup of W lanes (64, 256 or 1024), the instantiations and the layout of csrc/mcq_field.h, all in dynamic LDS:
//             red     32 dwords            the cross-wavefront half of the minimum
//             scan    16 x uint64          the wavefront totals of the prefix sum
//             win     2 dwords (+ pad)     the selected cell and its count
//             tab     512 dwords           the sweep's table row, staged once per sweep
//             field / occ / queens         csrc/mcq_field.h: 8- or 16-bit counts read as whole dwords, the occupancy bitmap with its
//                                          pad bits set, Q packed cells i << 10 | j << 5 | k
//           (137 504 bytes at N = 32, Q = N^3 - 1).  Taking a queen out and putting it back is that header's `put`: one 32-bit LDS
//           atomic per cell of the 13 lines.  Per queen update, between the two:
//             1. the minimum of S over the free cells: per lane, then __shfl_xor, then red;
//             2. the weights.  Cell-index order is part of the rule, so lane l owns the CONTIGUOUS run of R field dwords from l R on,
//                R = ceil(dwords / W) rounded up to an ODD number: ds_read_b32 banks by dword index mod 32 over each half of the
//                wavefront, and an odd stride sends the 32 lanes of a half to 32 different banks.  R <= 17 dwords = 34 cells at N = 32
//                and 7 dwords = 28 cells at N <= 19, so with entries of at most 2^24 (the rule, item 3) a lane's own sum stays below 2^30; the prefix over lanes is 64-bit: DPP row
//                shifts inside a row of 16 lanes, the four row totals by v_readlane, the wavefront totals through `scan`;
//             3. U = __umul64hi(x, W), and the ONE lane whose interval [P, P + sum) holds U walks its run again and writes the winner
//                to `win`.  Everything after that barrier is uniform over the workgroup, so every barrier is reached by all lanes;
//             4. one Philox block per two queens, the same counter in every lane (the compiler keeps it on the scalar unit).
//           A REPEATED placement is never put into the field: pairwise recount, written back unmoved.
//           At N <= 4 (at most 16 field dwords) most of the 64 lanes idle; several chains per wavefront are out of scope.
//   host    mcq_heatbath3d_host: the same rule with an int field per cell, a plain scan and 128-bit arithmetic for U.
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
using mcq_post::queens_of;
using mcq_post::philox_block;

thread_local char g_heatbath3d_err[256] = "";

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

template <int W, int BITS, int STEPS>
__global__ __launch_bounds__(W) void mcq_heatbath3d_kernel(Heatbath3dArgs a) {
    extern __shared__ uint32_t lds[];
    constexpr int CPD = 32 / BITS, SLOTS = 13 * STEPS;
    constexpr uint32_t MASK = (1u << BITS) - 1u;
    const int N = a.N, Q = a.Q, N2 = N * N, C = N2 * N, D = a.table_len;
    uint32_t* red = lds;
    unsigned long long* scan = (unsigned long long*)(lds + 32);
    uint32_t* win = lds + 64;
    uint32_t* tab = lds + HDR;
    const auto [field, occ, queens, fw, bw] = carve<BITS>(tab + TAB, C);
    const int tid = threadIdx.x;
    const long long ch = blockIdx.x;
    const uint8_t* in = a.state_in + ch * 3 * Q;
    uint8_t* out = a.state_out + ch * 3 * Q;
    uint8_t* bout = a.best_state ? a.best_state + ch * 3 * Q : nullptr;
    int32_t* hist = a.energy_hist ? a.energy_hist + ch * a.hist_stride : nullptr;

    for (int w = tid; w < fw + bw; w += W) field[w] = 0;  // (field and occ are adjacent)
    __syncthreads();
    if (tid == 0) {
        set_pad_bits(occ, bw, C);
        win[0] = win[1] = 0;
    }
    __syncthreads();
    int rep = 0;
    for (int q = tid; q < Q; q += W) rep |= load_queen(queens, occ, in, N, q);
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
            mcq_post::store_heatbath_figures(a, ch, e, e, e, 0, 0);
            if (a.flags) a.flags[ch] = MCQ_HEATBATH3D_REPEATED;
        }
        return;
    }

    for (int x = tid; x < Q * SLOTS; x += W) put_slot<W, BITS, STEPS>(field, queens, N, x);
    __syncthreads();
    int twoE = 0;
    for (int q = tid; q < Q; q += W) twoE += attackers_at<BITS>(field, N, queens[q]);
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
            const int pcell = cell_of(p, N);
            put<W, BITS, STEPS>(field, N, p, -1, tid, W, SLOTS);
            if (tid == 0) vacate(occ, pcell);
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
            const int a_min = (int)block_min<W, false>(m, red);
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
                t = packed_of(tcell, N, N2);
            }
            E += a_new - a_old;
            changed += tcell != pcell;
            put<W, BITS, STEPS>(field, N, t, +1, tid, W, SLOTS);
            if (tid == 0) occupy(occ, queens, q, t, tcell);
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
        mcq_post::store_heatbath_figures(a, ch, e_in, E, best, best_sweep, changed);
        if (a.flags) a.flags[ch] = 0;
    }
}

// what both entry points refuse
int check_heatbath3d(const mcq_heatbath3d* q) {
    if (!q) return fail(g_heatbath3d_err, MCQ_EINVAL, "mcq_heatbath3d: NULL parameter block");
    const int rc = mcq_post::check_full3d(g_heatbath3d_err, "heat-bath sweep", q->N, q->n_queens, (long long)q->n_chains);
    if (rc != MCQ_OK) return rc;
    if (q->n_sweeps < 0) return fail(g_heatbath3d_err, MCQ_EINVAL, "n_sweeps must be >= 0, got %lld", (long long)q->n_sweeps);
    if (q->first_sweep < 0) return fail(g_heatbath3d_err, MCQ_EINVAL, "first_sweep must be >= 0, got %lld", (long long)q->first_sweep);
    const uint64_t end = (uint64_t)q->first_sweep + (uint64_t)q->n_sweeps, Q = (uint64_t)queens_of(q);
    if (end > ((1ull << 62) - 1) / Q)
        return fail(g_heatbath3d_err, MCQ_EINVAL, "first_sweep + n_sweeps = %llu: the update index (first_sweep + n_sweeps) Q must stay below 2^62", (unsigned long long)end);
    if (q->table_len < 1 || q->table_len > MCQ_MAX_HEATBATH_TABLE)
        return fail(g_heatbath3d_err, MCQ_EINVAL, "table_len out of range [1, %d]: %lld", MCQ_MAX_HEATBATH_TABLE, (long long)q->table_len);
    if (!q->seeds) return fail(g_heatbath3d_err, MCQ_EINVAL, "seeds is required");
    if (!q->table && q->n_sweeps > 0) return fail(g_heatbath3d_err, MCQ_EINVAL, "table is required (n_sweeps rows of table_len words)");
    if (!q->state_in) return fail(g_heatbath3d_err, MCQ_EINVAL, "state_in is required");
    if (!q->state_out) return fail(g_heatbath3d_err, MCQ_EINVAL, "state_out is required");
    if (q->energy_hist && q->hist_stride < q->n_sweeps + 1)
        return fail(g_heatbath3d_err, MCQ_EINVAL, "hist_stride must be >= n_sweeps + 1 = %lld, got %lld", (long long)q->n_sweeps + 1, (long long)q->hist_stride);
    return MCQ_OK;
}

// what the host entry point refuses on top of that: it reads the table, which the device entry point cannot
int check_heatbath3d_table(const mcq_heatbath3d* q) {
    const long long D = (long long)q->table_len;
    for (long long s = 0; s < q->n_sweeps; s++)
        for (long long d = 0; d < D; d++)
            if (q->table[s * D + d] > (1u << MCQ_HEATBATH_WEIGHT_BITS))
                return fail(g_heatbath3d_err, MCQ_EINVAL, "table: the entry of sweep %lld at index %lld is %u, above 2^%d (a lane sums up to 34 entries in 32 bits)",
                            s, d, (unsigned)q->table[s * D + d], MCQ_HEATBATH_WEIGHT_BITS);
    return MCQ_OK;
}

// chains first .. last - 1 through the rule, with an int field per cell
void host_chains(const mcq_heatbath3d* q, long long first, long long last) {
    const int Q = queens_of(q), D = (int)q->table_len;
    HostField f(q->N, Q);
    const std::vector<int>& S = f.S;
    const std::vector<uint8_t>& occ = f.occ;
    const int C = f.C;
    for (long long ch = first; ch < last; ch++) {
        const uint8_t* in = q->state_in + ch * 3 * Q;
        uint8_t* bout = q->best_state ? q->best_state + ch * 3 * Q : nullptr;
        int32_t* hist = q->energy_hist ? q->energy_hist + ch * q->hist_stride : nullptr;
        const bool repeated = f.load(in);
        const int e_in = f.energy();
        int E = e_in, best = e_in;
        long long best_sweep = 0, changed = 0;
        if (hist) hist[0] = e_in;
        if (bout) f.store(bout);
        const uint32_t seed = q->seeds[ch];
        for (long long s = 0; s < q->n_sweeps; s++) {
            if (repeated) {
                if (hist) hist[s + 1] = e_in;
                continue;
            }
            const uint32_t* T = q->table + s * D;
            const uint64_t u0 = (uint64_t)(q->first_sweep + s) * (uint64_t)Q;
            for (int n = 0; n < Q; n++) {
                const int p = f.pos[(size_t)n];
                f.take_out(n);
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
                f.put_back(n, t);
            }
            if (hist) hist[s + 1] = E;
            if (E < best) {
                best = E;
                best_sweep = s + 1;
                if (bout) f.store(bout);
            }
        }
        f.store(q->state_out + ch * 3 * Q);
        mcq_post::store_heatbath_figures(*q, ch, e_in, E, best, best_sweep, changed);
        if (q->flags) q->flags[ch] = repeated ? MCQ_HEATBATH3D_REPEATED : 0;
    }
}

}  // namespace

extern "C" {

const char* mcq_heatbath3d_last_error(void) { return g_heatbath3d_err; }

int mcq_heatbath3d_host(const mcq_heatbath3d* q) {
    int rc = check_heatbath3d(q);
    if (rc == MCQ_OK) rc = check_heatbath3d_table(q);
    if (rc != MCQ_OK) return rc;
    mcq_post::for_chains(q->n_chains, [q](long long first, long long last) { host_chains(q, first, last); });
    return MCQ_OK;
}

int mcq_heatbath3d_device(const mcq_heatbath3d* q, void* hip_stream) {
    const int rc = check_heatbath3d(q);
    if (rc != MCQ_OK) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    const Heatbath3dArgs a{q->seeds, q->table, q->state_in, q->state_out, q->energy_in, q->energy_out, q->best_energy, q->best_sweep, q->best_state,
                           q->n_changed, q->energy_hist, q->flags, (long long)q->hist_stride, (long long)q->n_sweeps, (long long)q->first_sweep,
                           (int)q->table_len, (int)q->N, queens_of(q)};
    const hipError_t e = for_shape_of(a.N, [&](auto shape) {
        using S = decltype(shape);
        return launch<S>(mcq_heatbath3d_kernel<S::W, S::BITS, S::STEPS>, a, a.N, a.Q, HDR + TAB, (long long)q->n_chains, s);
    });
    if (e != hipSuccess) return fail(g_heatbath3d_err, MCQ_EDEVICE, "mcq_heatbath3d_device: %s", hipGetErrorString(e));
    return MCQ_OK;
}

}  // extern "C"
