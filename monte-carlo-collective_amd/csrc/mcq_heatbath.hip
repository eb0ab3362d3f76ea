// mcq_heatbath.hip -- heat-bath column sweeps of board placements (include/mcq.h: mcq_heatbath, where the rule is stated).  Like the quench
// (csrc/mcq_quench.hip) it sits outside the Metropolis sweep: placements in device memory in, placements and per-chain figures out.
//
//   kernel  the lanes of a GROUP are the candidate heights k of one column, as in the quench: 16, 32 or 64 lanes for N <= 16, 32, 64 and
//           64 lanes with two heights each (k and k + 64) beyond; a wavefront holds 4, 2 or 1 chains, a workgroup is one wavefront.
//           What differs from the quench is how a column's cells are fetched.  The chain keeps FOUR copies of its heights in LDS, one per
//           line family: by row, by board column, by diagonal (line i - j + N - 1) and by anti-diagonal (line i + j), each line NP bytes
//           long (NP = N rounded up to the instantiation's padding), indexed by j for the rows and by i for the other three, and holding
//           255 where the line has no cell.  The four lines through a column are then 4 NP contiguous bytes: they are fetched as whole
//           dwords (ds_read2_b32 / ds_read_b32, wider where the alignment is known), all issued before the first test, and the bytes are taken
//           apart in registers.  255 never counts (|255 - k| >= 128 > d), so the walk has no range checks and no branches; the column's own
//           cell sits on all four lines at distance 0 and counts once per line for k = h(c): a(c, k) = the count - 4 [k = h(c)].
//           The minimum runs over the group with DPP row rotations (16 lanes) and __shfl_xor beyond, the prefix sum with DPP row shifts
//           and the row totals, the selection is a ballot of C_k <= U, and one Philox block serves four columns.  The sweep's table row
//           is staged in LDS once per sweep.  A changed height is stored to the four copies by EVERY lane of the group (same address,
//           same value), so each lane's later reads are ordered behind its own store by program order, as in the quench.
//   host    mcq_heatbath_host: the same rule over host buffers, column by column with a plain table a[k].
//
// Built for gfx950 only, with csrc/mcq_hip.hip:  hipcc --offload-arch=gfx950 -O3 -ffp-contract=off
#include <hip/hip_runtime.h>

#include <climits>
#include <vector>

#include "../../include/mcq.h"
#include "mcq_columns.h"
#include "mcq_post.h"

namespace {

using mcq_columns::counter_offset;
using mcq_columns::group_min;
using mcq_columns::group_scan;
using mcq_columns::line_hits;
using mcq_post::fail;
using mcq_post::host_counts;
using mcq_post::philox_block;

thread_local char g_heatbath_err[256] = "";

struct HeatbathArgs {
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
    long long hist_stride;
    long long n_chains;
    long long n_sweeps;
    long long first_sweep;
    int table_len;
    int N;
};

template <int GW, int KPL, int NP>
__global__ __launch_bounds__(64) void mcq_heatbath_kernel(HeatbathArgs a) {
    constexpr int CPW = 64 / GW;       // chains per wavefront
    constexpr int NPW = NP / 4;        // dwords per line
    constexpr int FAM = NP * NPW;      // dwords of the row copy (and of the column copy); the two diagonal copies take 2 FAM each
    constexpr int CHAIN = 6 * FAM;
    __shared__ __attribute__((aligned(16))) uint32_t lds[CPW * CHAIN];
    __shared__ uint32_t tab[512];
    const int N = a.N, Q = N * N, D = a.table_len;
    const int lane = threadIdx.x & (GW - 1), grp = threadIdx.x / GW;
    const long long chain = (long long)blockIdx.x * CPW + grp;
    const bool valid = chain < a.n_chains;
    const long long ch = valid ? chain : a.n_chains - 1;  // a group beyond the last chain walks the last chain and writes nothing
    uint32_t* base = lds + grp * CHAIN;
    uint8_t* rows = (uint8_t*)base;
    uint8_t* cols = rows + 4 * FAM;
    uint8_t* diag = rows + 8 * FAM;
    uint8_t* anti = rows + 16 * FAM;
    for (int w = lane; w < CHAIN; w += GW) base[w] = 0xFFFFFFFFu;
    __syncthreads();
    const uint8_t* in = a.state_in + ch * Q;
    for (int c = lane; c < Q; c += GW) {
        const int v = in[c], i = c / N, j = c - i * N;
        const uint8_t hv = (uint8_t)(v < N ? v : N - 1);
        rows[i * NP + j] = hv;
        cols[j * NP + i] = hv;
        diag[(i - j + N - 1) * NP + i] = hv;
        anti[(i + j) * NP + i] = hv;
    }
    __syncthreads();
    if (valid && a.best_state) {  // until a sweep end is strictly lower: the (clamped) input
        uint8_t* out = a.best_state + ch * Q;
        for (int c = lane; c < Q; c += GW) {
            const int i = c / N;
            out[c] = rows[i * NP + (c - i * N)];
        }
    }
    const int k0 = lane, k1 = lane + 64;
    const uint32_t seed = a.seeds[ch];
    int32_t* hist = a.energy_hist ? a.energy_hist + ch * a.hist_stride : nullptr;

    int E = 0, e_in = 0, best = 0;
    long long best_sweep = 0, changed = 0;
    uint32_t rnd[4] = {0, 0, 0, 0};
    // sweep -1 is the recount of the input: the same walk with no update
    for (long long s = -1; s < a.n_sweeps; s++) {
        const bool recount = s < 0;
        if (!recount) {
            __syncthreads();
            const uint32_t* row = a.table + s * D;
            for (int d = threadIdx.x; d < D; d += 64) tab[d] = row[d];
            __syncthreads();
        }
        const unsigned long long w0 = recount ? 0ull : (unsigned long long)(a.first_sweep + s) * (unsigned long long)Q;
        int twoE = 0;
        for (int i = 0, c = 0; i < N; i++)
            for (int j = 0; j < N; j++, c++) {
                int c0 = 0, c1 = 0;
                const int dl = i - j + N - 1, al = i + j;
                line_hits<KPL, NP>(base + i * NPW, j, k0, k1, c0, c1);
                line_hits<KPL, NP>(base + FAM + j * NPW, i, k0, k1, c0, c1);
                line_hits<KPL, NP>(base + 2 * FAM + dl * NPW, i, k0, k1, c0, c1);
                line_hits<KPL, NP>(base + 4 * FAM + al * NPW, i, k0, k1, c0, c1);
                const int cur = rows[i * NP + j];
                c0 -= k0 == cur ? 4 : 0;
                if (KPL == 2) c1 -= k1 == cur ? 4 : 0;
                const int a_old = __shfl(KPL == 2 && cur >= 64 ? c1 : c0, cur & (GW - 1), GW);
                if (recount) {
                    twoE += a_old;
                    continue;
                }
                int m = k0 < N ? c0 : INT_MAX;
                if (KPL == 2) m = min(m, k1 < N ? c1 : INT_MAX);
                const int a_min = group_min<GW>(m);
                const uint32_t wt0 = k0 < N ? tab[k0 < N ? min(c0 - a_min, D - 1) : 0] : 0u;
                uint32_t W, C0 = group_scan<GW>(wt0, lane, W), C1 = 0;
                if (KPL == 2) {
                    const uint32_t wt1 = k1 < N ? tab[k1 < N ? min(c1 - a_min, D - 1) : 0] : 0u;
                    uint32_t W1;
                    C1 = W + group_scan<GW>(wt1, lane, W1);
                    W += W1;
                }
                const unsigned long long w = w0 + (unsigned)c;
                if ((w & 3) == 0 || c == 0) philox_block((uint32_t)(w >> 2), (uint32_t)(w >> 34), seed, 1u, rnd);
                const int e = (int)(w & 3);
                const uint32_t x = e == 0 ? rnd[0] : e == 1 ? rnd[1] : e == 2 ? rnd[2] : rnd[3];
                const uint32_t U = __umulhi(x, W);
                // the smallest k with C_k > U = the number of heights with C_k <= U (C is non-decreasing; a lane beyond N holds W > U)
                const unsigned long long gmask = GW == 64 ? ~0ull : ((1ull << GW) - 1);
                int kn = __popcll((__ballot(C0 <= U) >> (grp * GW)) & gmask);
                if (KPL == 2) kn += __popcll(__ballot(C1 <= U));
                kn = min(kn, N - 1);  // (only a table with T[0] = 0, W = 0, gets here: the last height, as in the host code)
                const int a_new = __shfl(KPL == 2 && kn >= 64 ? c1 : c0, kn & (GW - 1), GW);
                E += a_new - a_old;
                changed += kn != cur;
                const uint8_t hv = (uint8_t)kn;
                rows[i * NP + j] = hv;
                cols[j * NP + i] = hv;
                diag[dl * NP + i] = hv;
                anti[al * NP + i] = hv;
            }
        if (recount) {
            E = e_in = best = twoE >> 1;
            if (valid && hist && lane == 0) hist[0] = E;
            continue;
        }
        if (valid && hist && lane == 0) hist[s + 1] = E;
        if (E < best) {
            best = E;
            best_sweep = s + 1;
            if (valid && a.best_state) {
                uint8_t* out = a.best_state + ch * Q;
                for (int c = lane; c < Q; c += GW) {
                    const int i = c / N;
                    out[c] = rows[i * NP + (c - i * N)];
                }
            }
        }
    }
    if (!valid) return;
    uint8_t* out = a.state_out + ch * Q;
    for (int c = lane; c < Q; c += GW) {
        const int i = c / N;
        out[c] = rows[i * NP + (c - i * N)];
    }
    if (lane == 0) {
        mcq_post::store_heatbath_figures(a, ch, e_in, E, best, best_sweep, changed);
    }
}

// ---- the counter form, N <= MCQ_MAX_N_HEATBATH_COUNTERS (include/mcq.h: mcq_heatbath_counters_device) ----
// The same walk with the cells of a column never looked at.  The 12 line families of the cube that matter -- in-plane direction (0,1),
// (1,0), (1,1), (1,-1), height step 0, +1, -1 per cell along the line -- keep one byte each per line: the number of queens on it.
//   a(c, k) = the sum over the 12 families of the counter of the line through (i, j, k)  -  12 [k = h(c)]
// (the column's own queen lies on all 12 lines through its cell and on none through another cell of its column).  Where a counter is
// (counter_offset) and how large a chain's region -- these (6N - 2)(5N - 2) bytes and ONE copy of the heights -- is stands in
// csrc/mcq_columns.h, which csrc/mcq_temper.hip's counter kernel shares.  The counters are built once from the clamped input with 32-bit
// LDS atomics of 1 << 8 (byte in the dword): bytes of one dword belong to different lines, and a counter stays within 0 .. N <= 16, so a
// byte neither carries nor borrows.  A changed height moves 24
// counters before the next column is visited: lane f < 12 of the group owns family f and issues one atomic subtraction on the line
// through the old cell and one addition on the line through the new one.  The chains of a wavefront diverge on "changed"; there is no
// barrier inside that branch, and the LDS serves the instructions of one wavefront in their order, so the next column's reads see them.
template <int NP>
__global__ __launch_bounds__(64) void mcq_heatbath_counters_kernel(HeatbathArgs a) {
    constexpr int GW = 16, CPW = 64 / GW;
    constexpr int CNT = mcq_columns::counter_bytes(NP);                // bytes of counters; a multiple of 4 for NP = 8, 12, 16
    constexpr int CHAIN = mcq_columns::counter_region_bytes(NP);       // bytes of a chain's region: >= CNT + NP^2, = 64 mod 128
    static_assert(CNT % 4 == 0 && NP <= GW, "counter layout");
    __shared__ __attribute__((aligned(16))) uint32_t lds[CPW * CHAIN / 4];
    __shared__ uint32_t tab[512];
    const int N = a.N, Q = N * N, D = a.table_len;
    const int lane = threadIdx.x & (GW - 1), grp = threadIdx.x / GW;
    const long long chain = (long long)blockIdx.x * CPW + grp;
    const bool valid = chain < a.n_chains;
    const long long ch = valid ? chain : a.n_chains - 1;  // a group beyond the last chain walks the last chain and writes nothing
    uint32_t* cw = lds + grp * (CHAIN / 4);
    const uint8_t* cb = (const uint8_t*)cw;
    uint8_t* hts = (uint8_t*)cw + CNT;
    for (int w = lane; w < CNT / 4; w += GW) cw[w] = 0u;
    __syncthreads();
    const uint8_t* in = a.state_in + ch * Q;
    for (int c = lane; c < Q; c += GW) {
        const int v = in[c], i = c / N, j = c - i * N;
        const int hv = v < N ? v : N - 1;
        hts[c] = (uint8_t)hv;
#pragma unroll
        for (int f = 0; f < 12; f++) {
            const int b = counter_offset(f / 3, f % 3, i, j, N) + hv;
            atomicAdd(cw + (b >> 2), 1u << (8 * (b & 3)));
        }
    }
    __syncthreads();
    if (valid && a.best_state) {  // until a sweep end is strictly lower: the (clamped) input
        uint8_t* out = a.best_state + ch * Q;
        for (int c = lane; c < Q; c += GW) out[c] = hts[c];
    }
    const int k0 = lane, kr = min(lane, N - 1);  // a lane beyond N reads the counters of the last height and is left out below
    const int own_dir = lane / 3, own_step = lane - 3 * own_dir;  // lane f < 12 updates family f
    const uint32_t seed = a.seeds[ch];
    int32_t* hist = a.energy_hist ? a.energy_hist + ch * a.hist_stride : nullptr;

    int E = 0, e_in = 0, best = 0;
    long long best_sweep = 0, changed = 0;
    uint32_t rnd[4] = {0, 0, 0, 0};
    // sweep -1 is the recount of the input: the same walk with no update
    for (long long s = -1; s < a.n_sweeps; s++) {
        const bool recount = s < 0;
        if (!recount) {
            __syncthreads();
            const uint32_t* row = a.table + s * D;
            for (int d = threadIdx.x; d < D; d += 64) tab[d] = row[d];
            __syncthreads();
        }
        const unsigned long long w0 = recount ? 0ull : (unsigned long long)(a.first_sweep + s) * (unsigned long long)Q;
        int twoE = 0;
        for (int i = 0, c = 0; i < N; i++)
            for (int j = 0; j < N; j++, c++) {
                int c0 = 0;
#pragma unroll
                for (int f = 0; f < 12; f++) c0 += cb[counter_offset(f / 3, f % 3, i, j, N) + kr];
                const int cur = hts[c];
                c0 -= k0 == cur ? 12 : 0;
                const int a_old = __shfl(c0, cur, GW);
                if (recount) {
                    twoE += a_old;
                    continue;
                }
                const int a_min = group_min<GW>(k0 < N ? c0 : INT_MAX);
                const uint32_t wt0 = k0 < N ? tab[min(c0 - a_min, D - 1)] : 0u;
                uint32_t W;
                const uint32_t C0 = group_scan<GW>(wt0, lane, W);
                const unsigned long long w = w0 + (unsigned)c;
                if ((w & 3) == 0 || c == 0) philox_block((uint32_t)(w >> 2), (uint32_t)(w >> 34), seed, 1u, rnd);
                const int e = (int)(w & 3);
                const uint32_t x = e == 0 ? rnd[0] : e == 1 ? rnd[1] : e == 2 ? rnd[2] : rnd[3];
                const uint32_t U = __umulhi(x, W);
                // the smallest k with C_k > U = the number of heights with C_k <= U (C is non-decreasing; a lane beyond N holds W > U)
                int kn = __popcll((__ballot(C0 <= U) >> (grp * GW)) & ((1ull << GW) - 1));
                kn = min(kn, N - 1);  // (only a table with T[0] = 0, W = 0, gets here: the last height, as in the host code)
                const int a_new = __shfl(c0, kn, GW);
                E += a_new - a_old;
                changed += kn != cur;
                if (kn != cur && lane < 12) {
                    const int o = counter_offset(own_dir, own_step, i, j, N);
                    const int b0 = o + cur, b1 = o + kn;
                    atomicSub(cw + (b0 >> 2), 1u << (8 * (b0 & 3)));
                    atomicAdd(cw + (b1 >> 2), 1u << (8 * (b1 & 3)));
                }
                hts[c] = (uint8_t)kn;  // by every lane of the group: same address, same value
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // (no instruction: the compiler keeps the next column's reads behind the updates)
            }
        if (recount) {
            E = e_in = best = twoE >> 1;
            if (valid && hist && lane == 0) hist[0] = E;
            continue;
        }
        if (valid && hist && lane == 0) hist[s + 1] = E;
        if (E < best) {
            best = E;
            best_sweep = s + 1;
            if (valid && a.best_state) {
                uint8_t* out = a.best_state + ch * Q;
                for (int c = lane; c < Q; c += GW) out[c] = hts[c];
            }
        }
    }
    if (!valid) return;
    uint8_t* out = a.state_out + ch * Q;
    for (int c = lane; c < Q; c += GW) out[c] = hts[c];
    if (lane == 0) {
        mcq_post::store_heatbath_figures(a, ch, e_in, E, best, best_sweep, changed);
    }
}

// what every entry point refuses
int check_heatbath(const mcq_heatbath* q) {
    if (!q) return fail(g_heatbath_err, MCQ_EINVAL, "mcq_heatbath: NULL parameter block");
    if (q->mode != MCQ_MODE_BOARD) return fail(g_heatbath_err, MCQ_EINVAL, "mode: the heat-bath sweep runs boards only (MCQ_MODE_BOARD), got %d", (int)q->mode);
    if (q->N < MCQ_MIN_N || q->N > MCQ_MAX_N_BOARD) return fail(g_heatbath_err, MCQ_EINVAL, "N out of range [%d, %d]: %d", MCQ_MIN_N, MCQ_MAX_N_BOARD, (int)q->N);
    if (q->n_chains < 1 || q->n_chains > INT_MAX) return fail(g_heatbath_err, MCQ_EINVAL, "n_chains out of range [1, 2^31 - 1]: %lld", (long long)q->n_chains);
    if (q->n_sweeps < 0) return fail(g_heatbath_err, MCQ_EINVAL, "n_sweeps must be >= 0, got %lld", (long long)q->n_sweeps);
    if (q->first_sweep < 0) return fail(g_heatbath_err, MCQ_EINVAL, "first_sweep must be >= 0, got %lld", (long long)q->first_sweep);
    const uint64_t end = (uint64_t)q->first_sweep + (uint64_t)q->n_sweeps, Q = (uint64_t)q->N * (uint64_t)q->N;
    if (end > (uint64_t)INT64_MAX / Q)
        return fail(g_heatbath_err, MCQ_EINVAL, "first_sweep + n_sweeps = %llu: the word index (first_sweep + n_sweeps) N^2 must stay below 2^63", (unsigned long long)end);
    if (q->table_len < 1 || q->table_len > MCQ_MAX_HEATBATH_TABLE)
        return fail(g_heatbath_err, MCQ_EINVAL, "table_len out of range [1, %d]: %lld", MCQ_MAX_HEATBATH_TABLE, (long long)q->table_len);
    if (!q->seeds) return fail(g_heatbath_err, MCQ_EINVAL, "seeds is required");
    if (!q->table && q->n_sweeps > 0) return fail(g_heatbath_err, MCQ_EINVAL, "table is required (n_sweeps rows of table_len words)");
    if (!q->state_in) return fail(g_heatbath_err, MCQ_EINVAL, "state_in is required");
    if (!q->state_out) return fail(g_heatbath_err, MCQ_EINVAL, "state_out is required");
    if (q->energy_hist && q->hist_stride < q->n_sweeps + 1)
        return fail(g_heatbath_err, MCQ_EINVAL, "hist_stride must be >= n_sweeps + 1 = %lld, got %lld", (long long)q->n_sweeps + 1, (long long)q->hist_stride);
    return MCQ_OK;
}

// what the host entry point refuses on top of that: it reads the table, which the device entry points cannot
int check_heatbath_table(const mcq_heatbath* q) {
    const long long D = (long long)q->table_len;
    for (long long s = 0; s < q->n_sweeps; s++)
        for (long long d = 0; d < D; d++)
            if (q->table[s * D + d] > (1u << MCQ_HEATBATH_WEIGHT_BITS))
                return fail(g_heatbath_err, MCQ_EINVAL, "table: the entry of sweep %lld at index %lld is %u, above 2^%d (W must stay below 2^32 at N = 128)",
                            s, d, (unsigned)q->table[s * D + d], MCQ_HEATBATH_WEIGHT_BITS);
    return MCQ_OK;
}

template <int GW, int KPL, int NP>
void launch_heatbath(const HeatbathArgs& a, hipStream_t s) {
    constexpr int CPW = 64 / GW;
    hipLaunchKernelGGL((mcq_heatbath_kernel<GW, KPL, NP>), dim3((unsigned)((a.n_chains + CPW - 1) / CPW)), dim3(64), 0, s, a);
}

template <int NP>
void launch_heatbath_counters(const HeatbathArgs& a, hipStream_t s) {
    hipLaunchKernelGGL((mcq_heatbath_counters_kernel<NP>), dim3((unsigned)((a.n_chains + 3) / 4)), dim3(64), 0, s, a);
}

HeatbathArgs heatbath_args(const mcq_heatbath* q) {
    return HeatbathArgs{q->seeds, q->table, q->state_in, q->state_out, q->energy_in, q->energy_out, q->best_energy, q->best_sweep, q->best_state,
                        q->n_changed, q->energy_hist, (long long)q->hist_stride, (long long)q->n_chains, (long long)q->n_sweeps,
                        (long long)q->first_sweep, (int)q->table_len, (int)q->N};
}

}  // namespace

extern "C" {

const char* mcq_heatbath_last_error(void) { return g_heatbath_err; }

int mcq_heatbath_host(const mcq_heatbath* q) {
    int rc = check_heatbath(q);
    if (rc == MCQ_OK) rc = check_heatbath_table(q);
    if (rc != MCQ_OK) return rc;
    const int N = q->N, Q = N * N, D = (int)q->table_len;
    std::vector<uint8_t> h((size_t)Q);
    std::vector<int> a((size_t)N);
    std::vector<uint32_t> C((size_t)N);
    for (long long ch = 0; ch < q->n_chains; ch++) {
        const uint8_t* in = q->state_in + ch * Q;
        for (int c = 0; c < Q; c++) h[(size_t)c] = (uint8_t)(in[c] < N ? in[c] : N - 1);
        long long twoE = 0;
        for (int c = 0; c < Q; c++) {
            host_counts(h.data(), N, c / N, c % N, a.data());
            twoE += a[h[(size_t)c]];
        }
        const int e_in = (int)(twoE / 2);
        int E = e_in, best = e_in;
        long long best_sweep = 0, changed = 0;
        int32_t* hist = q->energy_hist ? q->energy_hist + ch * q->hist_stride : nullptr;
        if (hist) hist[0] = e_in;
        if (q->best_state)
            for (int c = 0; c < Q; c++) q->best_state[ch * Q + c] = h[(size_t)c];
        const uint32_t seed = q->seeds[ch];
        for (long long s = 0; s < q->n_sweeps; s++) {
            const uint32_t* T = q->table + s * D;
            const uint64_t w0 = (uint64_t)(q->first_sweep + s) * (uint64_t)Q;
            for (int c = 0; c < Q; c++) {
                host_counts(h.data(), N, c / N, c % N, a.data());
                int a_min = a[0];
                for (int k = 1; k < N; k++) a_min = a[k] < a_min ? a[k] : a_min;
                uint32_t sum = 0;
                for (int k = 0; k < N; k++) {
                    const int d = a[k] - a_min;
                    sum += T[d < D - 1 ? d : D - 1];
                    C[(size_t)k] = sum;
                }
                const uint64_t w = w0 + (uint64_t)c;
                uint32_t r[4];
                philox_block((uint32_t)(w >> 2), (uint32_t)(w >> 34), seed, 1u, r);
                const uint32_t U = (uint32_t)(((uint64_t)r[w & 3] * (uint64_t)sum) >> 32);
                int kn = 0;
                while (kn < N - 1 && C[(size_t)kn] <= U) kn++;  // (a table with T[0] = 0 gives W = 0: the last height, nothing leaves the arrays)
                const int cur = h[(size_t)c];
                E += a[kn] - a[cur];
                changed += kn != cur;
                h[(size_t)c] = (uint8_t)kn;
            }
            if (hist) hist[s + 1] = E;
            if (E < best) {
                best = E;
                best_sweep = s + 1;
                if (q->best_state)
                    for (int c = 0; c < Q; c++) q->best_state[ch * Q + c] = h[(size_t)c];
            }
        }
        uint8_t* out = q->state_out + ch * Q;
        for (int c = 0; c < Q; c++) out[c] = h[(size_t)c];
        mcq_post::store_heatbath_figures(*q, ch, e_in, E, best, best_sweep, changed);
    }
    return MCQ_OK;
}

int mcq_heatbath_device(const mcq_heatbath* q, void* hip_stream) {
    const int rc = check_heatbath(q);
    if (rc != MCQ_OK) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    const HeatbathArgs a = heatbath_args(q);
    const int N = q->N;
    if (N <= 8) launch_heatbath<16, 1, 8>(a, s);
    else if (N <= 12) launch_heatbath<16, 1, 12>(a, s);
    else if (N <= 16) launch_heatbath<16, 1, 16>(a, s);
    else if (N <= 24) launch_heatbath<32, 1, 24>(a, s);
    else if (N <= 32) launch_heatbath<32, 1, 32>(a, s);
    else if (N <= 64) launch_heatbath<64, 1, 64>(a, s);
    else launch_heatbath<64, 2, 128>(a, s);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(g_heatbath_err, MCQ_EDEVICE, "mcq_heatbath_device: %s", hipGetErrorString(e));
    return MCQ_OK;
}

int mcq_heatbath_counters_device(const mcq_heatbath* q, void* hip_stream) {
    const int rc = check_heatbath(q);
    if (rc != MCQ_OK) return rc;
    if (q->N > MCQ_MAX_N_HEATBATH_COUNTERS)
        return fail(g_heatbath_err, MCQ_EINVAL, "N = %d: the counter form of the heat-bath sweep runs N <= %d (MCQ_MAX_N_HEATBATH_COUNTERS); mcq_heatbath_device runs every N",
                             (int)q->N, MCQ_MAX_N_HEATBATH_COUNTERS);
    hipStream_t s = (hipStream_t)hip_stream;
    const HeatbathArgs a = heatbath_args(q);
    const int N = q->N;
    if (N <= 8) launch_heatbath_counters<8>(a, s);
    else if (N <= 12) launch_heatbath_counters<12>(a, s);
    else launch_heatbath_counters<16>(a, s);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(g_heatbath_err, MCQ_EDEVICE, "mcq_heatbath_counters_device: %s", hipGetErrorString(e));
    return MCQ_OK;
}

}  // extern "C"
