// mcq_quench3d.hip -- quench of full_3d placements: the deterministic zero-temperature descent of Q queens in the N^3 cube to a local
// minimum under single-queen moves (include/mcq.h: mcq_quench3d, where the rule is stated).  It sits outside the sweep like
// csrc/mcq_quench.hip: placements in device memory in, placements and per-chain figures out, nothing goes to the host.
//
//   design  a queen has N^3 targets, so nothing walks lines per candidate.  A chain keeps the ATTACK FIELD S(t) = the number of queens
//           that hold or attack cell t, one entry per cell.  Visiting queen q at p: take q out (S -= 1 on p and on the in-bounds cells
//           of the 13 lines through p), and a(q, t) IS S(t) for every t; one argmin over the free cells on the key S << 16 | cell;
//           put q back at the winner the same way.  O(N^3 / lanes + 13 N) per queen.  A queen with a(q, p) = 0 is skipped: no cell
//           can hold less.
//   kernel  one chain per workgroup of W lanes (64, 256 or 1024: one, four or sixteen wavefronts), all in LDS:
//             red     32 dwords  the cross-wavefront half of the reductions
//             field   one byte per cell while 13 (N - 1) + 1 <= 255 (N <= 19), 16 bits beyond (64 KiB at N = 32), read as whole dwords
//             occ     the occupancy bitmap, N^3 bits; the pad bits behind the last cell are set, so no argmin tests cell < N^3
//             queens  Q packed cells i << 10 | j << 5 | k, 16 bits each (132 KiB with everything at N = 32, Q = N^3 - 1)
//           The lines through p meet only in p, so one queen's update touches distinct cells, but two cells share a dword: the update
//           is a 32-bit LDS atomic add of +-1 << the cell's bit offset.  A byte never carries: it holds at most 13 (N - 1) + 1, and
//           the cell a queen is taken from counted that queen.  A lane's slot of an update is (direction, signed step), STEPS = 32
//           or 64 steps per direction, so the slot decodes with shifts.
//           Every branch on the chain's data (skip, move, end of the descent) is uniform over the workgroup, so every barrier is
//           reached by all lanes.  A REPEATED placement (two queens in one cell after clamping) breaks the byte bound and is never
//           put into the field: its counts come from a pairwise scan, Q^2 / W tests per lane, and it is written back unmoved.
//   host    mcq_quench3d_host: the same rule with an int field per cell and a plain scan of the cube.
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

thread_local char g_quench3d_err[256] = "";

int quench3d_fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_quench3d_err, sizeof g_quench3d_err, fmt, ap);
    va_end(ap);
    return code;
}

struct Quench3dArgs {
    const uint8_t* state_in;
    uint8_t* state_out;
    int32_t* energy_in;
    int32_t* energy_out;
    int32_t* n_moves;
    int32_t* n_passes;
    uint16_t* conflicts;
    int32_t* flags;
    long long max_passes;
    int N;
    int Q;
};

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

template <int W>
__device__ __forceinline__ uint32_t block_min(uint32_t v, uint32_t* red) {
    for (int o = 32; o; o >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, o, 64));
    if (W == 64) return v;
    __syncthreads();  // the readers of the reduction before this one are done with red
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

template <int W, int BITS, int STEPS>
__global__ __launch_bounds__(W) void mcq_quench3d_kernel(Quench3dArgs a) {
    extern __shared__ uint32_t lds[];
    constexpr int CPD = 32 / BITS, SLOTS = 13 * STEPS;
    const int N = a.N, Q = a.Q, N2 = N * N, C = N2 * N;
    const int fw = (C + CPD - 1) / CPD, bw = (C + 31) / 32;
    uint32_t* red = lds;
    uint32_t* field = lds + 32;
    uint32_t* occ = field + fw;
    uint16_t* queens = (uint16_t*)(occ + bw);
    const int tid = threadIdx.x;
    const long long ch = blockIdx.x;
    const uint8_t* in = a.state_in + ch * 3 * Q;
    uint8_t* out = a.state_out + ch * 3 * Q;

    for (int w = tid; w < fw + bw; w += W) field[w] = 0;  // (field and occ are adjacent)
    __syncthreads();
    if (tid == 0 && (C & 31)) occ[bw - 1] = ~0u << (C & 31);  // the pad bits: never a candidate
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

    if (repeated) {
        int twoE = 0;
        for (int q = tid; q < Q; q += W) {
            const int p = queens[q];
            int n = 0;
            for (int o = 0; o < Q; o++) n += attacks(p, queens[o]);
            n -= 1;  // itself
            twoE += n;
            if (a.conflicts) a.conflicts[ch * Q + q] = (uint16_t)n;
            out[3 * q] = (uint8_t)(p >> 10), out[3 * q + 1] = (uint8_t)((p >> 5) & 31), out[3 * q + 2] = (uint8_t)(p & 31);
        }
        twoE = block_sum<W>(twoE, red);
        if (tid == 0) {
            if (a.energy_in) a.energy_in[ch] = twoE >> 1;
            if (a.energy_out) a.energy_out[ch] = twoE >> 1;
            if (a.n_moves) a.n_moves[ch] = 0;
            if (a.n_passes) a.n_passes[ch] = 0;
            if (a.flags) a.flags[ch] = MCQ_QUENCH3D_REPEATED;
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

    int E = e_in, moves = 0, passes = 0;
    for (;;) {
        int moved = 0;
        for (int q = 0; q < Q; q++) {
            const int p = queens[q];
            const int pcell = ((p >> 10) * N + ((p >> 5) & 31)) * N + (p & 31);
            const int now = field_at<BITS>(field, pcell) - 1;
            if (now == 0) continue;  // (uniform: every lane read the same entries)
            __syncthreads();         // every lane has read S(p) before the queen is taken out
            put<W, BITS, STEPS>(field, N, p, -1, tid, W, SLOTS);
            if (tid == 0) occ[pcell >> 5] &= ~(1u << (pcell & 31));
            __syncthreads();
            uint32_t key = ~0u;
            for (int w = tid; w < fw; w += W) {
                const uint32_t v = field[w];
                const uint32_t o = occ[(w * CPD) >> 5] >> ((w * CPD) & 31);
#pragma unroll
                for (int b = 0; b < CPD; b++)
                    if (!((o >> b) & 1u)) key = min(key, ((v >> (b * BITS)) & ((1u << BITS) - 1u)) << 16 | (uint32_t)(w * CPD + b));
            }
            key = block_min<W>(key, red);
            const int best = (int)(key >> 16);
            int t = p, tcell = pcell;
            if (best < now) {
                tcell = (int)(key & 0xffffu);
                const int ti = tcell / N2, tj = (tcell - ti * N2) / N;
                t = ti << 10 | tj << 5 | (tcell - ti * N2 - tj * N);
                E += best - now;
                moved++;
            }
            __syncthreads();  // every lane has read queens[q] and the whole field before the queen goes back
            put<W, BITS, STEPS>(field, N, t, +1, tid, W, SLOTS);
            if (tid == 0) {
                occ[tcell >> 5] |= 1u << (tcell & 31);
                queens[q] = (uint16_t)t;
            }
            __syncthreads();
        }
        passes++;
        moves += moved;
        // (passes > e_in cannot happen -- every moving pass lowers E --: it only bounds the loop should the rule ever be broken)
        if (moved == 0 || (a.max_passes > 0 && passes >= a.max_passes) || passes > e_in) break;
    }

    for (int q = tid; q < Q; q += W) {
        const int p = queens[q];
        out[3 * q] = (uint8_t)(p >> 10), out[3 * q + 1] = (uint8_t)((p >> 5) & 31), out[3 * q + 2] = (uint8_t)(p & 31);
        if (a.conflicts) a.conflicts[ch * Q + q] = (uint16_t)(field_at<BITS>(field, ((p >> 10) * N + ((p >> 5) & 31)) * N + (p & 31)) - 1);
    }
    if (tid == 0) {
        if (a.energy_in) a.energy_in[ch] = e_in;
        if (a.energy_out) a.energy_out[ch] = E;
        if (a.n_moves) a.n_moves[ch] = moves;
        if (a.n_passes) a.n_passes[ch] = passes;
        if (a.flags) a.flags[ch] = 0;
    }
}

int queens_of(const mcq_quench3d* q) { return q->n_queens == 0 ? q->N * q->N : q->n_queens; }

// what both entry points refuse
int check_quench3d(const mcq_quench3d* q) {
    if (!q) return quench3d_fail(MCQ_EINVAL, "mcq_quench3d: NULL parameter block");
    if (q->N > MCQ_MAX_N_QUENCH3D && q->N <= MCQ_MAX_N)
        return quench3d_fail(MCQ_EINVAL, "N out of range [%d, %d]: %d (the full_3d quench stops at N = %d, where a cell index fits 15 bits; the sweep runs to %d)",
                             MCQ_MIN_N, MCQ_MAX_N_QUENCH3D, (int)q->N, MCQ_MAX_N_QUENCH3D, MCQ_MAX_N);
    if (q->N < MCQ_MIN_N || q->N > MCQ_MAX_N_QUENCH3D) return quench3d_fail(MCQ_EINVAL, "N out of range [%d, %d]: %d", MCQ_MIN_N, MCQ_MAX_N_QUENCH3D, (int)q->N);
    const int cells = q->N * q->N * q->N;
    if (q->n_queens != 0 && (q->n_queens < 2 || q->n_queens > cells - 1))
        return quench3d_fail(MCQ_EINVAL, "n_queens out of range [2, N^3 - 1 = %d] (0 = N^2): %d", cells - 1, (int)q->n_queens);
    if (q->n_chains < 1 || q->n_chains > INT_MAX) return quench3d_fail(MCQ_EINVAL, "n_chains out of range [1, 2^31 - 1]: %lld", (long long)q->n_chains);
    if (q->max_passes < 0) return quench3d_fail(MCQ_EINVAL, "max_passes must be >= 0 (0 = no limit), got %lld", (long long)q->max_passes);
    if (!q->state_in) return quench3d_fail(MCQ_EINVAL, "state_in is required");
    if (!q->state_out) return quench3d_fail(MCQ_EINVAL, "state_out is required");
    return MCQ_OK;
}

template <int W, int BITS, int STEPS>
hipError_t launch_quench3d(const Quench3dArgs& a, long long n_chains, hipStream_t s) {
    const int cells = a.N * a.N * a.N, cpd = 32 / BITS;
    const size_t bytes = 4 * (size_t)(32 + (cells + cpd - 1) / cpd + (cells + 31) / 32 + (a.Q + 1) / 2);
    if (bytes > 32 * 1024) {  // (the default limit is 64 KiB with the kernel's static LDS; a chain at N = 32 takes up to 132 KiB)
        const hipError_t e = hipFuncSetAttribute((const void*)mcq_quench3d_kernel<W, BITS, STEPS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((mcq_quench3d_kernel<W, BITS, STEPS>), dim3((unsigned)n_chains), dim3(W), bytes, s, a);
    return hipGetLastError();
}

// chains first .. last - 1 through the rule, with an int field per cell
void host_chains(const mcq_quench3d* q, long long first, long long last) {
    const int N = q->N, Q = queens_of(q), N2 = N * N, C = N2 * N;
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
    for (long long ch = first; ch < last; ch++) {
        const uint8_t* in = q->state_in + ch * 3 * Q;
        uint8_t* out = q->state_out + ch * 3 * Q;
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
        int E = e_in, moves = 0, passes = 0;
        while (!repeated) {
            int moved = 0;
            for (int n = 0; n < Q; n++) {
                const int p = pos[(size_t)n], now = S[(size_t)p] - 1;
                if (now == 0) continue;  // no cell can hold less
                put(p, -1);
                occ[(size_t)p] = 0;
                int t = -1;
                for (int c = 0; c < C; c++)
                    if (!occ[(size_t)c] && (t < 0 || S[(size_t)c] < S[(size_t)t])) t = c;  // strictly: the smallest cell of the minimum
                if (S[(size_t)t] < now) {
                    E += S[(size_t)t] - now;
                    moved++;
                } else {
                    t = p;
                }
                put(t, +1);
                occ[(size_t)t] = 1;
                pos[(size_t)n] = t;
            }
            passes++;
            moves += moved;
            if (moved == 0 || (q->max_passes > 0 && passes >= q->max_passes)) break;
        }
        for (int n = 0; n < Q; n++) {
            const int p = pos[(size_t)n];
            if (q->conflicts) q->conflicts[ch * Q + n] = (uint16_t)(S[(size_t)p] - 1);
            out[3 * n] = (uint8_t)(p / N2), out[3 * n + 1] = (uint8_t)((p / N) % N), out[3 * n + 2] = (uint8_t)(p % N);
        }
        if (q->energy_in) q->energy_in[ch] = e_in;
        if (q->energy_out) q->energy_out[ch] = E;
        if (q->n_moves) q->n_moves[ch] = moves;
        if (q->n_passes) q->n_passes[ch] = passes;
        if (q->flags) q->flags[ch] = repeated ? MCQ_QUENCH3D_REPEATED : 0;
    }
}

}  // namespace

extern "C" {

const char* mcq_quench3d_last_error(void) { return g_quench3d_err; }

int mcq_quench3d_host(const mcq_quench3d* q) {
    const int rc = check_quench3d(q);
    if (rc != MCQ_OK) return rc;
    // chains do not interact: a few threads share them (a test compares 65 536 chains with the kernel)
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

int mcq_quench3d_device(const mcq_quench3d* q, void* hip_stream) {
    const int rc = check_quench3d(q);
    if (rc != MCQ_OK) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    const Quench3dArgs a{q->state_in, q->state_out, q->energy_in, q->energy_out, q->n_moves, q->n_passes, q->conflicts, q->flags,
                         (long long)q->max_passes, (int)q->N, queens_of(q)};
    // the instantiation table: lanes per chain, field width, steps per direction of an update (2 N - 1 <= STEPS)
    hipError_t e;
    if (q->N <= 12) e = launch_quench3d<64, 8, 32>(a, (long long)q->n_chains, s);
    else if (q->N <= 19) e = launch_quench3d<256, 8, 64>(a, (long long)q->n_chains, s);
    else e = launch_quench3d<1024, 16, 64>(a, (long long)q->n_chains, s);
    if (e != hipSuccess) return quench3d_fail(MCQ_EDEVICE, "mcq_quench3d_device: %s", hipGetErrorString(e));
    return MCQ_OK;
}

}  // extern "C"
