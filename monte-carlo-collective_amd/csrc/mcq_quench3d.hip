// mcq_quench3d.hip -- quench of full_3d placements: the deterministic zero-temperature descent of Q queens in the N^3 cube to a local
// minimum under single-queen moves (include/mcq.h: mcq_quench3d, where the rule is stated).  It sits outside the sweep like
// csrc/mcq_quench.hip: placements in device memory in, placements and per-chain figures out, nothing goes to the host.
//
//   design  a queen has N^3 targets, so nothing walks lines per candidate.  A chain keeps the ATTACK FIELD S(t) = the number of queens
//           that hold or attack cell t, one entry per cell (csrc/mcq_field.h: the layout, the update, the byte bound, a repeated
//           placement, and the host form).  Visiting queen q at p: take q out, and a(q, t) IS S(t) for every t; one argmin over the
//           free cells on the key S << 16 | cell; put q back at the winner the same way.  O(N^3 / lanes + 13 N) per queen.  A queen
//           with a(q, p) = 0 is skipped: no cell can hold less.
//   kernel  one chain per workgroup of W lanes, all in LDS: red, 32 dwords, the cross-wavefront half of the reductions, then the
//           field, occ and the queens.
//           Every branch on the chain's data (skip, move, end of the descent) is uniform over the workgroup, so every barrier is
//           reached by all lanes.  A REPEATED placement is recounted pair by pair and written back unmoved.
//   host    mcq_quench3d_host: the same rule with an int field per cell and a plain scan of the cube.
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
using mcq_post::queens_of;

thread_local char g_quench3d_err[256] = "";

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

template <int W, int BITS, int STEPS>
__global__ __launch_bounds__(W) void mcq_quench3d_kernel(Quench3dArgs a) {
    extern __shared__ uint32_t lds[];
    constexpr int CPD = 32 / BITS, SLOTS = 13 * STEPS;
    const int N = a.N, Q = a.Q, N2 = N * N, C = N2 * N;
    uint32_t* red = lds;
    const auto [field, occ, queens, fw, bw] = carve<BITS>(lds + 32, C);
    const int tid = threadIdx.x;
    const long long ch = blockIdx.x;
    const uint8_t* in = a.state_in + ch * 3 * Q;
    uint8_t* out = a.state_out + ch * 3 * Q;

    for (int w = tid; w < fw + bw; w += W) field[w] = 0;  // (field and occ are adjacent)
    __syncthreads();
    if (tid == 0) set_pad_bits(occ, bw, C);
    __syncthreads();
    int rep = 0;
    for (int q = tid; q < Q; q += W) rep |= load_queen(queens, occ, in, N, q);
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
            store_queen(out, q, p);
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

    for (int x = tid; x < Q * SLOTS; x += W) put_slot<W, BITS, STEPS>(field, queens, N, x);
    __syncthreads();
    int twoE = 0;
    for (int q = tid; q < Q; q += W) twoE += attackers_at<BITS>(field, N, queens[q]);
    const int e_in = block_sum<W>(twoE, red) >> 1;

    int E = e_in, moves = 0, passes = 0;
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
            const int best = (int)(key >> 16);
            int t = p, tcell = pcell;
            if (best < now) {
                tcell = (int)(key & 0xffffu);
                t = packed_of(tcell, N, N2);
                E += best - now;
                moved++;
            }
            __syncthreads();  // every lane has read queens[q] and the whole field before the queen goes back
            put<W, BITS, STEPS>(field, N, t, +1, tid, W, SLOTS);
            if (tid == 0) occupy(occ, queens, q, t, tcell);
            __syncthreads();
        }
        passes++;
        moves += moved;
        // (passes > e_in cannot happen -- every moving pass lowers E --: it only bounds the loop should the rule ever be broken)
        if (moved == 0 || (a.max_passes > 0 && passes >= a.max_passes) || passes > e_in) break;
    }

    for (int q = tid; q < Q; q += W) {
        const int p = queens[q];
        // (written out: store_queen and attackers_at here changed the kernel's code)
        out[3 * q] = (uint8_t)(p >> 10), out[3 * q + 1] = (uint8_t)((p >> 5) & 31), out[3 * q + 2] = (uint8_t)(p & 31);
        if (a.conflicts) a.conflicts[ch * Q + q] = (uint16_t)(field_at<BITS>(field, ((p >> 10) * N + ((p >> 5) & 31)) * N + (p & 31)) - 1);
    }
    if (tid == 0) {
        mcq_post::store_quench_figures(a, ch, e_in, E, moves, passes);
        if (a.flags) a.flags[ch] = 0;
    }
}

// what both entry points refuse
int check_quench3d(const mcq_quench3d* q) {
    if (!q) return fail(g_quench3d_err, MCQ_EINVAL, "mcq_quench3d: NULL parameter block");
    const int rc = mcq_post::check_full3d(g_quench3d_err, "quench", q->N, q->n_queens, (long long)q->n_chains);
    if (rc != MCQ_OK) return rc;
    if (q->max_passes < 0) return fail(g_quench3d_err, MCQ_EINVAL, "max_passes must be >= 0 (0 = no limit), got %lld", (long long)q->max_passes);
    if (!q->state_in) return fail(g_quench3d_err, MCQ_EINVAL, "state_in is required");
    if (!q->state_out) return fail(g_quench3d_err, MCQ_EINVAL, "state_out is required");
    return MCQ_OK;
}

// chains first .. last - 1 through the rule, with an int field per cell
void host_chains(const mcq_quench3d* q, long long first, long long last) {
    const int Q = queens_of(q);
    HostField f(q->N, Q);
    const std::vector<int>& S = f.S;
    for (long long ch = first; ch < last; ch++) {
        const bool repeated = f.load(q->state_in + ch * 3 * Q);
        const int e_in = f.energy();
        int E = e_in, moves = 0, passes = 0;
        while (!repeated) {
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
            if (moved == 0 || (q->max_passes > 0 && passes >= q->max_passes)) break;
        }
        if (q->conflicts)
            for (int n = 0; n < Q; n++) q->conflicts[ch * Q + n] = (uint16_t)(S[(size_t)f.pos[(size_t)n]] - 1);
        f.store(q->state_out + ch * 3 * Q);
        mcq_post::store_quench_figures(*q, ch, e_in, E, moves, passes);
        if (q->flags) q->flags[ch] = repeated ? MCQ_QUENCH3D_REPEATED : 0;
    }
}

}  // namespace

extern "C" {

const char* mcq_quench3d_last_error(void) { return g_quench3d_err; }

int mcq_quench3d_host(const mcq_quench3d* q) {
    const int rc = check_quench3d(q);
    if (rc != MCQ_OK) return rc;
    mcq_post::for_chains(q->n_chains, [q](long long first, long long last) { host_chains(q, first, last); });
    return MCQ_OK;
}

int mcq_quench3d_device(const mcq_quench3d* q, void* hip_stream) {
    const int rc = check_quench3d(q);
    if (rc != MCQ_OK) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    const Quench3dArgs a{q->state_in, q->state_out, q->energy_in, q->energy_out, q->n_moves, q->n_passes, q->conflicts, q->flags,
                         (long long)q->max_passes, (int)q->N, queens_of(q)};
    const hipError_t e = for_shape_of(a.N, [&](auto shape) {
        using S = decltype(shape);
        return launch<S>(mcq_quench3d_kernel<S::W, S::BITS, S::STEPS>, a, a.N, a.Q, 32, (long long)q->n_chains, s);
    });
    if (e != hipSuccess) return fail(g_quench3d_err, MCQ_EDEVICE, "mcq_quench3d_device: %s", hipGetErrorString(e));
    return MCQ_OK;
}

}  // extern "C"
