// mcq_quench.hip -- quench: the deterministic zero-temperature descent of board placements to a local minimum under single-height
// moves (include/mcq.h: mcq_quench, where the rule is stated).  It sits outside the sweep like csrc/mcq_resume.hip and
// csrc/mcq_population.hip: placements in device memory in, placements and per-chain figures out, nothing goes to the host.
//
//   kernel  the lanes of a GROUP are the candidate heights k of one column: 16, 32 or 64 lanes for N <= 16, 32, 64, and 64 lanes with
//           two heights each (k and k + 64) beyond.  A wavefront holds 4, 2 or 1 chains, a workgroup is one wavefront, and there is no
//           barrier.  The chain's N^2 heights sit in LDS.  For column c = (i, j) the group walks the <= 4 (N - 1) columns of its row,
//           its column and its two diagonals: every lane of the group reads the same height h' (a broadcast read) and counts
//           |h' - k| in {0, d}.  The argmin runs over the group with __shfl_xor on the key count << 8 | k, so the smallest k wins a
//           tie; a(c, h(c)) comes from the lane that holds the current height.
//           Every loop bound is the same for all chains of the wavefront (one N, row-major columns), so the walk is scalar control
//           flow; a chain that has finished stays in step and is masked, and the wavefront ends when its last chain does.
//           The new height is stored by EVERY lane of the group (same address, same value), not by one: each lane's later reads of it
//           are then ordered behind its own store by program order alone, with no fence to get wrong; LDS operations of one wavefront
//           execute in order.
//           Two walks beyond the descent: one before it for energy_in (the recount), one behind it, when asked for, for the
//           conflict map of the output.
//   host    mcq_quench_host: the same rule over host buffers, column by column with a plain table a[k].
//
// Built for gfx950 only, with csrc/mcq_hip.hip:  hipcc --offload-arch=gfx950 -O3 -ffp-contract=off
#include <hip/hip_runtime.h>

#include <climits>
#include <vector>

#include "../../include/mcq.h"
#include "mcq_post.h"

namespace {

using mcq_post::fail;
using mcq_post::host_counts;

thread_local char g_quench_err[256] = "";

struct QuenchArgs {
    const uint8_t* state_in;
    uint8_t* state_out;
    int32_t* energy_in;
    int32_t* energy_out;
    int32_t* n_moves;
    int32_t* n_passes;
    uint16_t* conflicts;
    long long n_chains;
    long long max_passes;
    int N;
};

// a(c, k) of column (i, j) for this lane's heights k0 (and k1 with two heights per lane), from the heights h of the chain
template <int KPL>
__device__ __forceinline__ void column_counts(const uint8_t* h, int N, int i, int j, int k0, int k1, int& c0, int& c1) {
    c0 = 0, c1 = 0;
    auto hit = [&](int hp, int d) {
        const int a0 = abs(hp - k0);
        c0 += (a0 == 0) | (a0 == d);
        if (KPL == 2) {
            const int a1 = abs(hp - k1);
            c1 += (a1 == 0) | (a1 == d);
        }
    };
    const uint8_t* row = h + i * N;
    for (int jj = 0; jj < N; jj++) {  // the row, and the two diagonal cells of board column jj
        if (jj == j) continue;
        const int d = jj > j ? jj - j : j - jj;
        hit(row[jj], d);
        if (i + d < N) hit(h[(i + d) * N + jj], d);
        if (i - d >= 0) hit(h[(i - d) * N + jj], d);
    }
    for (int ii = 0; ii < N; ii++) {  // the board column
        if (ii == i) continue;
        hit(h[ii * N + j], ii > i ? ii - i : i - ii);
    }
}

template <int GW, int KPL, int NMAX>
__global__ __launch_bounds__(64) void mcq_quench_kernel(QuenchArgs a) {
    constexpr int CPW = 64 / GW;  // chains per wavefront
    __shared__ uint8_t heights[CPW * NMAX * NMAX];
    const int N = a.N, Q = N * N;
    const int lane = threadIdx.x & (GW - 1), grp = threadIdx.x / GW;
    const long long chain = (long long)blockIdx.x * CPW + grp;
    const bool valid = chain < a.n_chains;
    const long long ch = valid ? chain : a.n_chains - 1;  // a group beyond the last chain walks the last chain and writes nothing
    uint8_t* h = heights + grp * Q;
    const uint8_t* in = a.state_in + ch * Q;
    for (int c = lane; c < Q; c += GW) {
        const int v = in[c];
        h[c] = (uint8_t)(v < N ? v : N - 1);
    }
    const int k0 = lane, k1 = lane + 64;

    // the count at the current height of column c, given the lane's counts
    auto at_current = [&](int cur, int c0, int c1) { return __shfl(KPL == 2 && cur >= 64 ? c1 : c0, cur & (GW - 1), GW); };

    int twoE = 0;
    for (int i = 0, c = 0; i < N; i++)
        for (int j = 0; j < N; j++, c++) {
            int c0, c1;
            column_counts<KPL>(h, N, i, j, k0, k1, c0, c1);
            twoE += at_current(h[c], c0, c1);
        }
    const int e_in = twoE >> 1;
    int E = e_in, moves = 0, passes = 0;
    bool active = true;
    while (__any(active)) {
        int moved = 0;
        for (int i = 0, c = 0; i < N; i++)
            for (int j = 0; j < N; j++, c++) {
                int c0, c1;
                column_counts<KPL>(h, N, i, j, k0, k1, c0, c1);
                int key = k0 < N ? (c0 << 8) | k0 : INT_MAX;
                if (KPL == 2) key = min(key, k1 < N ? (c1 << 8) | k1 : INT_MAX);
                for (int o = GW >> 1; o; o >>= 1) key = min(key, __shfl_xor(key, o, GW));
                const int cur = h[c];
                const int now = at_current(cur, c0, c1), best = key >> 8;
                if (active && best < now) {
                    h[c] = (uint8_t)(key & 255);
                    E += best - now;
                    moved++;
                }
            }
        if (active) {
            passes++;
            moves += moved;
            // (passes > e_in cannot happen -- every moving pass lowers E --: it only bounds the loop should the rule ever be broken)
            if (moved == 0 || (a.max_passes > 0 && passes >= a.max_passes) || passes > e_in) active = false;
        }
    }
    if (a.conflicts) {
        uint16_t* out = a.conflicts + ch * Q;
        for (int i = 0, c = 0; i < N; i++)
            for (int j = 0; j < N; j++, c++) {
                int c0, c1;
                column_counts<KPL>(h, N, i, j, k0, k1, c0, c1);
                const int now = at_current(h[c], c0, c1);
                if (valid && lane == 0) out[c] = (uint16_t)now;
            }
    }
    if (!valid) return;
    uint8_t* out = a.state_out + ch * Q;
    for (int c = lane; c < Q; c += GW) out[c] = h[c];
    if (lane == 0) {
        mcq_post::store_quench_figures(a, ch, e_in, E, moves, passes);
    }
}

// what both entry points refuse
int check_quench(const mcq_quench* q) {
    if (!q) return fail(g_quench_err, MCQ_EINVAL, "mcq_quench: NULL parameter block");
    if (q->mode != MCQ_MODE_BOARD) return fail(g_quench_err, MCQ_EINVAL, "mode: the quench runs boards only (MCQ_MODE_BOARD), got %d", (int)q->mode);
    if (q->N < MCQ_MIN_N || q->N > MCQ_MAX_N_BOARD) return fail(g_quench_err, MCQ_EINVAL, "N out of range [%d, %d]: %d", MCQ_MIN_N, MCQ_MAX_N_BOARD, (int)q->N);
    if (q->n_chains < 1 || q->n_chains > INT_MAX) return fail(g_quench_err, MCQ_EINVAL, "n_chains out of range [1, 2^31 - 1]: %lld", (long long)q->n_chains);
    if (q->max_passes < 0) return fail(g_quench_err, MCQ_EINVAL, "max_passes must be >= 0 (0 = no limit), got %lld", (long long)q->max_passes);
    if (!q->state_in) return fail(g_quench_err, MCQ_EINVAL, "state_in is required");
    if (!q->state_out) return fail(g_quench_err, MCQ_EINVAL, "state_out is required");
    return MCQ_OK;
}

template <int GW, int KPL, int NMAX>
void launch_quench(const QuenchArgs& a, hipStream_t s) {
    constexpr int CPW = 64 / GW;
    hipLaunchKernelGGL((mcq_quench_kernel<GW, KPL, NMAX>), dim3((unsigned)((a.n_chains + CPW - 1) / CPW)), dim3(64), 0, s, a);
}

}  // namespace

extern "C" {

const char* mcq_quench_last_error(void) { return g_quench_err; }

int mcq_quench_host(const mcq_quench* q) {
    const int rc = check_quench(q);
    if (rc != MCQ_OK) return rc;
    const int N = q->N, Q = N * N;
    std::vector<uint8_t> h((size_t)Q);
    std::vector<int> a((size_t)N);
    for (long long ch = 0; ch < q->n_chains; ch++) {
        const uint8_t* in = q->state_in + ch * Q;
        for (int c = 0; c < Q; c++) h[(size_t)c] = (uint8_t)(in[c] < N ? in[c] : N - 1);
        long long twoE = 0;
        for (int c = 0; c < Q; c++) {
            host_counts(h.data(), N, c / N, c % N, a.data());
            twoE += a[h[(size_t)c]];
        }
        const int e_in = (int)(twoE / 2);
        int E = e_in, moves = 0, passes = 0;
        for (;;) {
            int moved = 0;
            for (int c = 0; c < Q; c++) {
                host_counts(h.data(), N, c / N, c % N, a.data());
                int best = 0;
                for (int k = 1; k < N; k++)
                    if (a[k] < a[best]) best = k;  // strictly: the smallest k of the minimum
                const int now = a[h[(size_t)c]];
                if (a[best] < now) {
                    h[(size_t)c] = (uint8_t)best;
                    E += a[best] - now;
                    moved++;
                }
            }
            passes++;
            moves += moved;
            if (moved == 0 || (q->max_passes > 0 && passes >= q->max_passes)) break;
        }
        if (q->conflicts)
            for (int c = 0; c < Q; c++) {
                host_counts(h.data(), N, c / N, c % N, a.data());
                q->conflicts[ch * Q + c] = (uint16_t)a[h[(size_t)c]];
            }
        uint8_t* out = q->state_out + ch * Q;
        for (int c = 0; c < Q; c++) out[c] = h[(size_t)c];
        mcq_post::store_quench_figures(*q, ch, e_in, E, moves, passes);
    }
    return MCQ_OK;
}

int mcq_quench_device(const mcq_quench* q, void* hip_stream) {
    const int rc = check_quench(q);
    if (rc != MCQ_OK) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    const QuenchArgs a{q->state_in, q->state_out, q->energy_in, q->energy_out, q->n_moves, q->n_passes, q->conflicts,
                       (long long)q->n_chains, (long long)q->max_passes, (int)q->N};
    if (q->N <= 16) launch_quench<16, 1, 16>(a, s);
    else if (q->N <= 32) launch_quench<32, 1, 32>(a, s);
    else if (q->N <= 64) launch_quench<64, 1, 64>(a, s);
    else launch_quench<64, 2, 128>(a, s);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(g_quench_err, MCQ_EDEVICE, "mcq_quench_device: %s", hipGetErrorString(e));
    return MCQ_OK;
}

}  // extern "C"
