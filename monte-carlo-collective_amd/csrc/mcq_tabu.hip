// mcq_tabu.hip -- tabu search of board placements: every iteration takes the best admissible single-height move of a conflicting column,
// also when it raises the energy, and forbids the height it left for a while (include/mcq.h: mcq_tabu, where the rule is stated).  The
// table a(c, k), its rows and `apply` are those of csrc/mcq_hop.hip: the board table of csrc/mcq_table.h; what this file adds is the walk
// over the table with a stamp per (c, k), as one launch.
//
//   kernel  one chain per wavefront, one wavefront per workgroup, as in the hops.  LDS holds the WHOLE table a(c, k) in the
//           layout of csrc/mcq_table.h, the stamps T(c, k) as one uint16 per entry in rows of TS bytes (like S a multiple of 4 with an
//           odd number of dwords: a lane per column reads its table row and its stamp row as dwords without bank conflicts), the
//           chain's N^2 heights and its best placement (N^2 bytes, written to global memory once, at the end).  The table is built
//           ONCE per launch; a move goes through `apply`, which touches at most 6 entries in each of the <= 4 (N - 1) aligned columns.
//           STAMPS are kept relative to a base, first_iter to begin with, that moves by 2^15 every 2^15 iterations with a saturating
//           subtraction over the stamp table: a stamp at or below the base is tabu for no later iteration and reads as 0 in tabu_out,
//           so nothing is lost, and base-relative stamps stay below 2^15 + 2^14 (tabu_in: below 2^16).
//           ITERATION: the Philox block is computed from values that are uniform over the wavefront.  Each lane takes its columns 64
//           apart and forms one 32-bit key (delta + 124) << 15 | rho over its admissible candidates (|delta| <= 4 (N - 1) = 124,
//           rho < N^3 <= 2^15); a __shfl_xor butterfly picks the smallest.  F is a popcount of ballots.  Then one stamp store, `apply`,
//           E and the counters.  The barriers are those of a one-wavefront workgroup (csrc/mcq_table.h).
//   host    mcq_tabu_host: the same rule over host buffers with plain loops, 64-bit absolute stamps and a table of ints that follows
//           every move; threaded over chains.
//
// Built for gfx950 only, with csrc/mcq_hip.hip:  hipcc --offload-arch=gfx950 -O3 -ffp-contract=off
#include <hip/hip_runtime.h>

#include <climits>
#include <vector>

#include "../../include/mcq.h"
#include "mcq_post.h"
#include "mcq_table.h"

namespace {

using mcq_post::fail;
using mcq_post::philox_block;
using mcq_post::rebase2;
using mcq_post::REBASE;

thread_local char g_tabu_err[256] = "";

constexpr uint32_t TABU_KEY_WORD = 7u;  // key word 1 of the chain's Philox stream: 0 - 6 are the sweep's, the heat baths', the tempered sweeps' and the hops'
constexpr int DELTA_BIAS = 124;         // 4 (MCQ_MAX_N_QUENCH_PAIRS - 1): delta + DELTA_BIAS >= 0
constexpr int RHO_BITS = 15;            // rho < 32^3
constexpr uint32_t KEY_NONE = 0xFFFFFFFFu;

struct TabuArgs {
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
    long long hist_stride;
    long long n_chains;
    long long n_iters;
    long long first_iter;
    int tenure;
    int tenure_rand;
    int tenure_conf;
    int N;
};

// the per-chain figures, by one lane or by the host: `a` is the kernel's argument struct or the parameter block
template <class A>
__host__ __device__ __forceinline__ void store_tabu_figures(const A& a, long long ch, int e_in, int E, int B, long long best_iter, long long moves,
                                                            long long aspired, long long uphill, long long stalled) {
    if (a.energy_in) a.energy_in[ch] = e_in;
    if (a.energy_out) a.energy_out[ch] = E;
    if (a.best_energy) a.best_energy[ch] = B;
    if (a.best_iter) a.best_iter[ch] = best_iter;
    if (a.n_moves) a.n_moves[ch] = moves;
    if (a.n_aspired) a.n_aspired[ch] = aspired;
    if (a.n_uphill) a.n_uphill[ch] = uphill;
    if (a.n_stalled) a.n_stalled[ch] = stalled;
}

// the words of iteration g: the tie offset o and the tenure's jitter
__host__ __device__ __forceinline__ void tabu_draw(uint32_t seed, unsigned long long g, int N3, int tenure_rand, int& o, int& jitter) {
    uint32_t r[4];
    philox_block((uint32_t)g, (uint32_t)(g >> 32), seed, TABU_KEY_WORD, r);
    o = (int)(((unsigned long long)r[0] * (unsigned)N3) >> 32);
    jitter = (int)(((unsigned long long)r[1] * (unsigned)(tenure_rand + 1)) >> 32);
}

template <int NP>
constexpr int tabu_lds_bytes() {
    return NP * NP * (4 * ((NP / 4) | 1) + 4 * ((NP / 2) | 1) + 2);
}

template <int NP>
__global__ __launch_bounds__(64) void mcq_tabu_kernel(TabuArgs a) {
    using R = mcq_table::Rows<NP>;
    constexpr int QP = R::QP, SW = R::SW, S = R::S, RW = R::RW;
    constexpr int TW = (NP / 2) | 1, TS = 2 * TW;   // dwords and uint16s of a stamp row
    __shared__ uint32_t tab32[QP * SW];
    __shared__ uint32_t stamp32[QP * TW];
    __shared__ uint8_t h[QP], best[QP];
    static_assert(sizeof(tab32) + sizeof(stamp32) + sizeof(h) + sizeof(best) == tabu_lds_bytes<NP>(), "the LDS of a chain, as the host checks it");
    const uint8_t* tab = reinterpret_cast<const uint8_t*>(tab32);
    uint16_t* stamp = reinterpret_cast<uint16_t*>(stamp32);
    const int N = a.N, Q = N * N, N3 = Q * N;
    const int lane = threadIdx.x;
    const long long ch = blockIdx.x;
    const uint32_t seed = a.seeds[ch];
    const uint8_t* in = a.state_in + ch * Q;
    for (int c = lane; c < Q; c += 64) {
        const uint8_t hc = mcq_table::clamped(in[c], N);
        h[c] = hc, best[c] = hc;
    }
    mcq_table::fill<NP>(tab32, Q, lane);
    for (int w = lane; w < Q * TW; w += 64) stamp32[w] = 0u;
    __syncthreads();
    if (a.tabu_in) {
        const uint16_t* ti = a.tabu_in + ch * N3;
        for (int e = lane; e < N3; e += 64) {
            const int c = e / N, k = e - c * N;
            stamp[c * TS + k] = ti[e];
        }
    }
    mcq_table::build<NP>(tab32, h, N, lane);
    const int e_in = mcq_table::energy<NP>(tab32, h, N, lane);
    int E = e_in, B = e_in;
    if (a.best_floor) B = min(B, a.best_floor[ch]);
    long long moves = 0, aspired = 0, uphill = 0, stalled = 0, best_iter = 0;
    if (a.energy_hist && lane == 0) a.energy_hist[ch * a.hist_stride] = E;

    long long t_base = 0;  // the iteration of the call at which the stamps' base lies
    for (long long t = 0; t < a.n_iters; t++) {
        if (t - t_base == REBASE) {
            for (int w = lane; w < Q * TW; w += 64) stamp32[w] = rebase2(stamp32[w]);
            t_base = t;
            __syncthreads();
        }
        const int now_rel = (int)(t - t_base);  // g less the base: a stamp above it is tabu
        int o, jitter;
        tabu_draw(seed, (unsigned long long)(a.first_iter + t), N3, a.tenure_rand, o, jitter);

        uint32_t key = KEY_NONE;
        int F = 0;
        for (int base = 0; base < Q; base += 64) {
            const int c = base + lane;
            bool conflicting = false;
            if (c < Q) {
                const int hc = h[c], now = tab[c * S + hc];
                conflicting = now > 0;
                if (conflicting) {
                    const uint32_t* row = tab32 + c * SW;
                    const uint32_t* srow = stamp32 + c * TW;
                    const int rho0 = c * N - o;
#pragma unroll
                    for (int w = 0; w < RW; w++) {
                        const uint32_t v = row[w], s0 = srow[2 * w], s1 = srow[2 * w + 1];
#pragma unroll
                        for (int b = 0; b < 4; b++) {
                            const int k = 4 * w + b;
                            const int delta = (int)((v >> (8 * b)) & 255u) - now;
                            const int st = (int)(((b < 2 ? s0 : s1) >> (16 * (b & 1))) & 0xFFFFu);
                            const bool admissible = st <= now_rel || E + delta < B;
                            int rho = rho0 + k;
                            rho += rho < 0 ? N3 : 0;
                            const uint32_t cand = ((uint32_t)(delta + DELTA_BIAS) << RHO_BITS) | (uint32_t)rho;
                            if (k < N && k != hc && admissible) key = min(key, cand);
                        }
                    }
                }
            }
            F += __popcll(__ballot(conflicting));
        }
        for (int x = 32; x; x >>= 1) key = min(key, (uint32_t)__shfl_xor((int)key, x));

        if (key == KEY_NONE) {
            stalled++;
        } else {
            const int delta = (int)(key >> RHO_BITS) - DELTA_BIAS;
            int idx = (int)(key & ((1u << RHO_BITS) - 1u)) + o;
            idx -= idx >= N3 ? N3 : 0;
            const int c = idx / N, k = idx - c * N, ho = h[c];
            const int L = a.tenure + jitter + ((a.tenure_conf * F) >> 4);
            aspired += (int)stamp[c * TS + k] > now_rel;
            uphill += delta > 0;
            moves++;
            if (lane == 0) stamp[c * TS + ho] = (uint16_t)(now_rel + 1 + L);
            mcq_table::apply<NP>(tab32, h, N, lane, c, k);
            E += delta;
            if (E < B) {
                B = E, best_iter = t + 1;
                for (int cc = lane; cc < Q; cc += 64) best[cc] = h[cc];
            }
        }
        if (a.energy_hist && lane == 0) a.energy_hist[ch * a.hist_stride + (t + 1)] = E;
    }
    __syncthreads();

    uint8_t* out = a.state_out + ch * Q;
    for (int c = lane; c < Q; c += 64) out[c] = h[c];
    if (a.best_state) {
        uint8_t* bs = a.best_state + ch * Q;
        for (int c = lane; c < Q; c += 64) bs[c] = best[c];
    }
    if (a.tabu_out) {
        const int end_rel = (int)(a.n_iters - t_base);  // first_iter + n_iters less the base
        uint16_t* to = a.tabu_out + ch * N3;
        for (int e = lane; e < N3; e += 64) {
            const int c = e / N, k = e - c * N, st = stamp[c * TS + k];
            to[e] = (uint16_t)(st > end_rel ? st - end_rel : 0);
        }
    }
    if (lane == 0) store_tabu_figures(a, ch, e_in, E, B, best_iter, moves, aspired, uphill, stalled);
}

int lds_bytes(int N) {
    return mcq_table::for_rows_of(N, [](auto rows) { return tabu_lds_bytes<decltype(rows)::NP>(); });
}

// what both entry points refuse
int check_tabu(const mcq_tabu* q) {
    if (!q) return fail(g_tabu_err, MCQ_EINVAL, "mcq_tabu: NULL parameter block");
    if (q->mode != MCQ_MODE_BOARD) return fail(g_tabu_err, MCQ_EINVAL, "mode: tabu search runs boards only (MCQ_MODE_BOARD), got %d", (int)q->mode);
    if (q->N < MCQ_MIN_N || q->N > MCQ_MAX_N_QUENCH_PAIRS)
        return fail(g_tabu_err, MCQ_EINVAL, "N out of range [%d, %d]: %d", MCQ_MIN_N, MCQ_MAX_N_QUENCH_PAIRS, (int)q->N);
    if (q->n_chains < 1 || q->n_chains > INT_MAX) return fail(g_tabu_err, MCQ_EINVAL, "n_chains out of range [1, 2^31 - 1]: %lld", (long long)q->n_chains);
    if (q->n_iters < 0) return fail(g_tabu_err, MCQ_EINVAL, "n_iters must be >= 0 (0 = the recount), got %lld", (long long)q->n_iters);
    if (q->first_iter < 0) return fail(g_tabu_err, MCQ_EINVAL, "first_iter must be >= 0, got %lld", (long long)q->first_iter);
    if ((unsigned long long)q->first_iter + (unsigned long long)q->n_iters >= (1ull << 63))
        return fail(g_tabu_err, MCQ_EINVAL, "iterations: first_iter + n_iters must stay below 2^63 (first_iter %lld, n_iters %lld)", (long long)q->first_iter,
                    (long long)q->n_iters);
    if (q->tenure < 0 || q->tenure > MCQ_MAX_TABU_TENURE)
        return fail(g_tabu_err, MCQ_EINVAL, "tenure out of range [0, %d]: %d", MCQ_MAX_TABU_TENURE, (int)q->tenure);
    if (q->tenure_rand < 0 || q->tenure_rand > MCQ_MAX_TABU_TENURE_RAND)
        return fail(g_tabu_err, MCQ_EINVAL, "tenure_rand out of range [0, %d]: %d", MCQ_MAX_TABU_TENURE_RAND, (int)q->tenure_rand);
    if (q->tenure_conf < 0 || q->tenure_conf > MCQ_MAX_TABU_TENURE_CONF)
        return fail(g_tabu_err, MCQ_EINVAL, "tenure_conf out of range [0, %d]: %d", MCQ_MAX_TABU_TENURE_CONF, (int)q->tenure_conf);
    if (!q->seeds) return fail(g_tabu_err, MCQ_EINVAL, "seeds is required");
    if (!q->state_in) return fail(g_tabu_err, MCQ_EINVAL, "state_in is required");
    if (!q->state_out) return fail(g_tabu_err, MCQ_EINVAL, "state_out is required");
    if (q->energy_hist && q->hist_stride < q->n_iters + 1)
        return fail(g_tabu_err, MCQ_EINVAL, "hist_stride must be >= n_iters + 1 = %lld, got %lld", (long long)q->n_iters + 1, (long long)q->hist_stride);
    if (q->best_state && (q->best_state == q->state_in || q->best_state == q->state_out))
        return fail(g_tabu_err, MCQ_EINVAL, "best_state must be distinct from state_in and state_out (it is written while they are in use)");
    if (lds_bytes(q->N) > MCQ_MAX_TABU_LDS)
        return fail(g_tabu_err, MCQ_EINVAL, "N = %d: a chain takes %d bytes of LDS, above the %d of a workgroup", (int)q->N, lds_bytes(q->N), MCQ_MAX_TABU_LDS);
    return MCQ_OK;
}

// one chain in host code: absolute 64-bit stamps, and a table of ints that follows every move
void host_chain(const mcq_tabu* q, long long ch) {
    const int N = q->N, Q = N * N, N3 = Q * N;
    std::vector<uint8_t> h((size_t)Q), best((size_t)Q);
    std::vector<int> A((size_t)N3);
    std::vector<long long> T((size_t)N3, 0LL);
    mcq_table::host_load(q->state_in + ch * Q, N, h.data());
    best = h;
    if (q->tabu_in)
        for (int e = 0; e < N3; e++) T[(size_t)e] = q->first_iter + (long long)q->tabu_in[ch * N3 + e];
    const int e_in = mcq_table::host_table(h.data(), N, A.data());
    int E = e_in, B = e_in;
    if (q->best_floor && q->best_floor[ch] < B) B = q->best_floor[ch];
    long long moves = 0, aspired = 0, uphill = 0, stalled = 0, best_iter = 0;
    int32_t* hist = q->energy_hist ? q->energy_hist + ch * q->hist_stride : nullptr;
    if (hist) hist[0] = E;
    const uint32_t seed = q->seeds[ch];
    for (long long t = 0; t < q->n_iters; t++) {
        const long long g = q->first_iter + t;
        int o, jitter;
        tabu_draw(seed, (unsigned long long)g, N3, q->tenure_rand, o, jitter);
        int F = 0, bd = INT_MAX, brho = INT_MAX, bc = -1, bk = -1;
        for (int c = 0; c < Q; c++) {
            const int* row = A.data() + (size_t)c * N;
            const int hc = h[(size_t)c];
            if (row[hc] == 0) continue;
            F++;
            for (int k = 0; k < N; k++) {
                if (k == hc) continue;
                const int delta = row[k] - row[hc];
                if (T[(size_t)c * N + k] > g && !(E + delta < B)) continue;
                const int rho = (c * N + k - o + N3) % N3;
                if (delta < bd || (delta == bd && rho < brho)) bd = delta, brho = rho, bc = c, bk = k;
            }
        }
        if (bc < 0) {
            stalled++;
        } else {
            const int ho = h[(size_t)bc], i = bc / N, j = bc % N;
            aspired += T[(size_t)bc * N + bk] > g;
            uphill += bd > 0;
            moves++;
            T[(size_t)bc * N + ho] = g + 1 + q->tenure + jitter + q->tenure_conf * F / 16;
            for (int c2 = 0; c2 < Q; c2++) {  // the rows of the aligned columns follow
                const int di = c2 / N - i, dj = c2 % N - j, adi = di < 0 ? -di : di, adj = dj < 0 ? -dj : dj;
                if (c2 == bc || !(di == 0 || dj == 0 || adi == adj)) continue;
                const int d = adi > adj ? adi : adj;
                int* row = A.data() + (size_t)c2 * N;
                for (int s = -1; s <= 1; s++) {
                    if (ho + s * d >= 0 && ho + s * d < N) row[ho + s * d]--;
                    if (bk + s * d >= 0 && bk + s * d < N) row[bk + s * d]++;
                }
            }
            h[(size_t)bc] = (uint8_t)bk;
            E += bd;
            if (E < B) B = E, best_iter = t + 1, best = h;
        }
        if (hist) hist[t + 1] = E;
    }
    uint8_t* out = q->state_out + ch * Q;
    for (int c = 0; c < Q; c++) out[c] = h[(size_t)c];
    if (q->best_state)
        for (int c = 0; c < Q; c++) q->best_state[ch * Q + c] = best[(size_t)c];
    if (q->tabu_out) {
        const long long end = q->first_iter + q->n_iters;
        for (int e = 0; e < N3; e++) q->tabu_out[ch * N3 + e] = (uint16_t)(T[(size_t)e] > end ? T[(size_t)e] - end : 0);
    }
    store_tabu_figures(*q, ch, e_in, E, B, best_iter, moves, aspired, uphill, stalled);
}

}  // namespace

extern "C" {

const char* mcq_tabu_last_error(void) { return g_tabu_err; }

int mcq_tabu_host(const mcq_tabu* q) {
    const int rc = check_tabu(q);
    if (rc != MCQ_OK) return rc;
    mcq_post::for_chains((long long)q->n_chains, [q](long long first, long long last) {
        for (long long ch = first; ch < last; ch++) host_chain(q, ch);
    });
    return MCQ_OK;
}

int mcq_tabu_device(const mcq_tabu* q, void* hip_stream) {
    const int rc = check_tabu(q);
    if (rc != MCQ_OK) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    const TabuArgs a{q->seeds, q->state_in, q->state_out, q->tabu_in, q->tabu_out, q->best_floor, q->energy_in, q->energy_out, q->best_energy,
                     q->best_iter, q->best_state, q->n_moves, q->n_aspired, q->n_uphill, q->n_stalled, q->energy_hist, (long long)q->hist_stride,
                     (long long)q->n_chains, (long long)q->n_iters, (long long)q->first_iter, (int)q->tenure, (int)q->tenure_rand,
                     (int)q->tenure_conf, (int)q->N};
    mcq_table::for_rows_of(q->N, [&](auto rows) {
        hipLaunchKernelGGL(mcq_tabu_kernel<decltype(rows)::NP>, dim3((unsigned)a.n_chains), dim3(64), 0, s, a);
    });
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(g_tabu_err, MCQ_EDEVICE, "mcq_tabu_device: %s", hipGetErrorString(e));
    return MCQ_OK;
}

}  // extern "C"
