// mcq_eo.hip -- extremal optimisation of board placements (tau-EO): every iteration ranks the columns by their local badness
// lambda(c) = a(c, h(c)), draws a rank from one table and moves the column at that rank unconditionally (include/mcq.h: mcq_eo, where the
// rule is stated).  The table a(c, k), its rows and `apply` are the board table of csrc/mcq_table.h, as in csrc/mcq_tabu.hip and
// csrc/mcq_relink.hip; what this file adds is the rank search over lambda, as one launch.
//
//   kernel  one chain per wavefront, one wavefront per workgroup.  LDS holds the WHOLE table a(c, k) in the layout of csrc/mcq_table.h,
//           the chain's N^2 heights, its best placement (N^2 bytes, written to global memory once, at the end) and rank_cdf, staged once
//           (it is uniform over the launch; at most N^2 - 1 dwords).  The table is built ONCE per launch; a move goes through `apply`.
//           ITERATION: the Philox block is computed from values that are uniform over the wavefront.  j is a popcount of ballots over
//           the staged rank_cdf.  Each lane gathers lambda of its columns 64 apart into registers (QP / 64 of them, -1 behind N^2).
//           THE RANK SEARCH sorts nothing: lambda < 128, so position j lies in the value class v = the largest v with
//           #{lambda >= v} > j, found by a bisection over the bits of v, each step a sum of popcounts of ballots (lambda >= v | bit);
//           the count of the last step that failed is #{lambda > v}, so m = j - #{lambda > v} is the ordinal inside the class in the
//           order of rho.  With n_lo the members of the class below o, that is the ordinal (m + n_lo) mod |class| in the order of c,
//           and the lane whose column is a member with that many members in front of it (ballots again, mbcnt inside a round) names c.
//           A bisection rather than a 128-bin LDS histogram with a suffix scan: by the compiler's instruction count the bisection is
//           the shorter kernel in five instantiations of six (DESIGN.md 4.24 has the figures), and the histogram costs a clear,
//           QP / 64 rounds of LDS atomics that serialise on a plateau (most columns share one lambda) and a scan with its waits, every
//           iteration; the bisection is at most 7 QP / 64 compares, all on registers, and takes no LDS beyond what the chain has.
//           HEIGHT: a lane per height reads the row of c; best = a __shfl_xor butterfly over (a(c, k) << 5 | (k - oh) mod N).  Then
//           `apply`, E and the counters.  The barriers are those of a one-wavefront workgroup (csrc/mcq_table.h); no scratch.
//   host    mcq_eo_host: the same rule over host buffers with plain loops: a table of ints that follows every move, and in every
//           iteration an explicit std::stable_sort of the columns by (-lambda, rho); threaded over chains.  It shares nothing with the
//           kernel's rank search.
//
// Built for gfx950 only, with csrc/mcq_hip.hip:  hipcc --offload-arch=gfx950 -O3 -ffp-contract=off
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <vector>

#include "../../include/mcq.h"
#include "mcq_post.h"
#include "mcq_table.h"

namespace {

using mcq_post::fail;
using mcq_post::philox_block;

thread_local char g_eo_err[256] = "";

constexpr uint32_t EO_KEY_WORD = 13u;  // key word 1 of the chain's Philox stream: 0 - 12 are taken (include/mcq.h)
constexpr int RHO_BITS = 5;            // (k - oh) mod N < 32
constexpr uint32_t KEY_NONE = 0xFFFFFFFFu;

struct EoArgs {
    const uint32_t* seeds;
    const uint32_t* rank_cdf;
    const uint8_t* state_in;
    uint8_t* state_out;
    const int32_t* best_floor;
    int32_t* energy_in;
    int32_t* energy_out;
    int32_t* best_energy;
    int64_t* best_iter;
    uint8_t* best_state;
    int64_t* n_moves;
    int64_t* n_uphill;
    int64_t* n_flat;
    int64_t* n_free;
    int64_t* n_idle;
    int32_t* energy_hist;
    long long hist_stride;
    long long n_chains;
    long long n_iters;
    long long first_iter;
    int move;
    int n_ranks;
    int N;
};

// the per-chain figures, by one lane or by the host: `a` is the kernel's argument struct or the parameter block
template <class A>
__host__ __device__ __forceinline__ void store_eo_figures(const A& a, long long ch, int e_in, int E, int B, long long best_iter, long long moves,
                                                          long long uphill, long long flat, long long free_moves, long long idle) {
    if (a.energy_in) a.energy_in[ch] = e_in;
    if (a.energy_out) a.energy_out[ch] = E;
    if (a.best_energy) a.best_energy[ch] = B;
    if (a.best_iter) a.best_iter[ch] = best_iter;
    if (a.n_moves) a.n_moves[ch] = moves;
    if (a.n_uphill) a.n_uphill[ch] = uphill;
    if (a.n_flat) a.n_flat[ch] = flat;
    if (a.n_free) a.n_free[ch] = free_moves;
    if (a.n_idle) a.n_idle[ch] = idle;
}

// the words of iteration g: x0 for the rank, the tie offsets o of the columns and oh of the heights, and the height k' of a random move
__host__ __device__ __forceinline__ void eo_draw(uint32_t seed, unsigned long long g, int N, uint32_t& x0, int& o, int& oh, int& kr) {
    uint32_t r[4];
    philox_block((uint32_t)g, (uint32_t)(g >> 32), seed, EO_KEY_WORD, r);
    x0 = r[0];
    o = (int)(((unsigned long long)r[1] * (unsigned)(N * N)) >> 32);
    oh = (int)(((unsigned long long)r[2] * (unsigned)N) >> 32);
    kr = (int)(((unsigned long long)r[3] * (unsigned)(N - 1)) >> 32);
}

template <int NP>
constexpr int eo_lds_bytes() {
    return NP * NP * (4 * ((NP / 4) | 1) + 6);
}

// the lanes of the wavefront below this one whose bit is set in b
__device__ __forceinline__ int ballot_prefix(unsigned long long b) {
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
}

template <int NP>
__global__ __launch_bounds__(64) void mcq_eo_kernel(EoArgs a) {
    using R = mcq_table::Rows<NP>;
    constexpr int QP = R::QP, SW = R::SW, S = R::S;
    constexpr int ROUNDS = (QP + 63) / 64;  // the columns of a lane, 64 apart
    __shared__ uint32_t tab32[QP * SW];
    __shared__ uint32_t cdf[QP];
    __shared__ uint8_t h[QP], best[QP];
    static_assert(sizeof(tab32) + sizeof(cdf) + sizeof(h) + sizeof(best) == eo_lds_bytes<NP>(), "the LDS of a chain, as the host checks it");
    const uint8_t* tab = reinterpret_cast<const uint8_t*>(tab32);
    const int N = a.N, Q = N * N, n_ranks = a.n_ranks;
    const int lane = threadIdx.x;
    const long long ch = blockIdx.x;
    const uint32_t seed = a.seeds[ch];
    for (int i = lane; i < n_ranks; i += 64) cdf[i] = a.rank_cdf[i];  // n_ranks <= Q - 1 < QP
    const int e_in = mcq_table::start<NP>(tab32, h, a.state_in + ch * Q, N, lane);
    for (int c = lane; c < Q; c += 64) best[c] = h[c];
    __syncthreads();
    int E = e_in, B = e_in;
    if (a.best_floor) B = min(B, a.best_floor[ch]);
    long long moves = 0, uphill = 0, flat = 0, free_moves = 0, idle = 0, best_iter = 0;
    if (a.energy_hist && lane == 0) a.energy_hist[ch * a.hist_stride] = E;
    int top_bit = 1;  // the highest bit of 4 (N - 1), the largest lambda
    while (2 * top_bit <= 4 * (N - 1)) top_bit *= 2;

    for (long long t = 0; t < a.n_iters; t++) {
        if (E == 0) {
            idle++;
            if (a.energy_hist && lane == 0) a.energy_hist[ch * a.hist_stride + (t + 1)] = E;
            continue;
        }
        uint32_t x0;
        int o, oh, kr;
        eo_draw(seed, (unsigned long long)(a.first_iter + t), N, x0, o, oh, kr);

        int j = 0;
        for (int base = 0; base < n_ranks; base += 64) {
            const int i = base + lane;
            j += __popcll(__ballot(i < n_ranks && cdf[i] <= x0));
        }

        int lam[ROUNDS];
#pragma unroll
        for (int r = 0; r < ROUNDS; r++) {
            const int c = 64 * r + lane;
            lam[r] = c < Q ? (int)tab[c * S + h[c]] : -1;
        }
        // the value class of position j: the largest v with #{lambda >= v} > j; `above` = #{lambda > v}
        int v = 0, above = 0;
        for (int bit = top_bit; bit; bit >>= 1) {
            int cnt = 0;
#pragma unroll
            for (int r = 0; r < ROUNDS; r++)
                if (64 * r < Q) cnt += __popcll(__ballot(lam[r] >= (v | bit)));
            if (cnt > j) v |= bit;
            else above = cnt;
        }
        // the class in the order of c: its size, and its members below o
        int size = 0, n_lo = 0;
#pragma unroll
        for (int r = 0; r < ROUNDS; r++) {
            if (64 * r < Q) {
                size += __popcll(__ballot(lam[r] == v));
                n_lo += __popcll(__ballot(lam[r] == v && 64 * r + lane < o));
            }
        }
        int want = j - above + n_lo;  // the ordinal in the order of rho, turned into the order of c
        want -= want >= size ? size : 0;
        int c = 0, run = 0;
#pragma unroll
        for (int r = 0; r < ROUNDS; r++) {
            if (64 * r < Q) {
                const bool member = lam[r] == v;
                const unsigned long long b = __ballot(member);
                const unsigned long long hit = __ballot(member && run + ballot_prefix(b) == want);
                if (hit) c = 64 * r + __ffsll(hit) - 1;
                run += __popcll(b);
            }
        }
        c = __builtin_amdgcn_readfirstlane(c);

        const int hc = h[c];
        const uint8_t* row = tab + c * S;
        int k, ak;
        if (a.move == MCQ_EO_MOVE_BEST) {
            uint32_t key = KEY_NONE;
            if (lane < N && lane != hc) {
                int rho = lane - oh;
                rho += rho < 0 ? N : 0;
                key = ((uint32_t)row[lane] << RHO_BITS) | (uint32_t)rho;
            }
            for (int x = 32; x; x >>= 1) key = min(key, (uint32_t)__shfl_xor((int)key, x));
            ak = (int)(key >> RHO_BITS);
            k = (int)(key & ((1u << RHO_BITS) - 1u)) + oh;
            k -= k >= N ? N : 0;
        } else {
            k = kr + (kr >= hc);
            ak = row[k];
        }
        const int delta = ak - v;  // lambda(c) = v
        moves++;
        uphill += delta > 0;
        flat += delta == 0;
        free_moves += v == 0;
        mcq_table::apply<NP>(tab32, h, N, lane, c, k);
        E += delta;
        if (E < B) {
            B = E, best_iter = t + 1;
            for (int cc = lane; cc < Q; cc += 64) best[cc] = h[cc];
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
    if (lane == 0) store_eo_figures(a, ch, e_in, E, B, best_iter, moves, uphill, flat, free_moves, idle);
}

int lds_bytes(int N) {
    return mcq_table::for_rows_of(N, [](auto rows) { return eo_lds_bytes<decltype(rows)::NP>(); });
}

// what both entry points refuse
int check_eo(const mcq_eo* q) {
    if (!q) return fail(g_eo_err, MCQ_EINVAL, "mcq_eo: NULL parameter block");
    if (q->mode != MCQ_MODE_BOARD) return fail(g_eo_err, MCQ_EINVAL, "mode: extremal optimisation runs boards only (MCQ_MODE_BOARD), got %d", (int)q->mode);
    if (q->N < MCQ_MIN_N || q->N > MCQ_MAX_N_QUENCH_PAIRS)
        return fail(g_eo_err, MCQ_EINVAL, "N out of range [%d, %d]: %d", MCQ_MIN_N, MCQ_MAX_N_QUENCH_PAIRS, (int)q->N);
    if (q->n_chains < 1 || q->n_chains > INT_MAX) return fail(g_eo_err, MCQ_EINVAL, "n_chains out of range [1, 2^31 - 1]: %lld", (long long)q->n_chains);
    if (q->n_iters < 0) return fail(g_eo_err, MCQ_EINVAL, "n_iters must be >= 0 (0 = the recount), got %lld", (long long)q->n_iters);
    if (q->first_iter < 0) return fail(g_eo_err, MCQ_EINVAL, "first_iter must be >= 0, got %lld", (long long)q->first_iter);
    if ((unsigned long long)q->first_iter + (unsigned long long)q->n_iters >= (1ull << 63))
        return fail(g_eo_err, MCQ_EINVAL, "iterations: first_iter + n_iters must stay below 2^63 (first_iter %lld, n_iters %lld)", (long long)q->first_iter,
                    (long long)q->n_iters);
    if (q->move != MCQ_EO_MOVE_BEST && q->move != MCQ_EO_MOVE_RANDOM)
        return fail(g_eo_err, MCQ_EINVAL, "move must be %d (best) or %d (random), got %d", MCQ_EO_MOVE_BEST, MCQ_EO_MOVE_RANDOM, (int)q->move);
    if (q->n_ranks < 0 || q->n_ranks > q->N * q->N - 1)
        return fail(g_eo_err, MCQ_EINVAL, "n_ranks out of range [0, N^2 - 1 = %d]: %d", (int)(q->N * q->N - 1), (int)q->n_ranks);
    if (q->n_ranks > 0 && !q->rank_cdf) return fail(g_eo_err, MCQ_EINVAL, "rank_cdf is required when n_ranks > 0 (n_ranks %d)", (int)q->n_ranks);
    if (!q->seeds) return fail(g_eo_err, MCQ_EINVAL, "seeds is required");
    if (!q->state_in) return fail(g_eo_err, MCQ_EINVAL, "state_in is required");
    if (!q->state_out) return fail(g_eo_err, MCQ_EINVAL, "state_out is required");
    if (q->energy_hist && q->hist_stride < q->n_iters + 1)
        return fail(g_eo_err, MCQ_EINVAL, "hist_stride must be >= n_iters + 1 = %lld, got %lld", (long long)q->n_iters + 1, (long long)q->hist_stride);
    if (q->best_state && (q->best_state == q->state_in || q->best_state == q->state_out))
        return fail(g_eo_err, MCQ_EINVAL, "best_state must be distinct from state_in and state_out (it is written while they are in use)");
    if (lds_bytes(q->N) > MCQ_MAX_EO_LDS)
        return fail(g_eo_err, MCQ_EINVAL, "N = %d: a chain takes %d bytes of LDS, above the %d of a workgroup", (int)q->N, lds_bytes(q->N), MCQ_MAX_EO_LDS);
    return MCQ_OK;
}

// one chain in host code: a table of ints that follows every move, and a stable sort of the columns in every iteration
void host_chain(const mcq_eo* q, long long ch) {
    const int N = q->N, Q = N * N;
    std::vector<uint8_t> h((size_t)Q), best((size_t)Q);
    std::vector<int> A((size_t)Q * N), lam((size_t)Q), rho((size_t)Q), order((size_t)Q);
    mcq_table::host_load(q->state_in + ch * Q, N, h.data());
    best = h;
    const int e_in = mcq_table::host_table(h.data(), N, A.data());
    int E = e_in, B = e_in;
    if (q->best_floor && q->best_floor[ch] < B) B = q->best_floor[ch];
    long long moves = 0, uphill = 0, flat = 0, free_moves = 0, idle = 0, best_iter = 0;
    int32_t* hist = q->energy_hist ? q->energy_hist + ch * q->hist_stride : nullptr;
    if (hist) hist[0] = E;
    const uint32_t seed = q->seeds[ch];
    for (long long t = 0; t < q->n_iters; t++) {
        if (E == 0) {
            idle++;
            if (hist) hist[t + 1] = E;
            continue;
        }
        uint32_t x0;
        int o, oh, kr;
        eo_draw(seed, (unsigned long long)(q->first_iter + t), N, x0, o, oh, kr);
        int j = 0;
        for (int i = 0; i < q->n_ranks; i++) j += q->rank_cdf[i] <= x0;
        for (int c = 0; c < Q; c++) {
            lam[(size_t)c] = A[(size_t)c * N + h[(size_t)c]];
            rho[(size_t)c] = (c - o + Q) % Q;
            order[(size_t)c] = c;
        }
        std::stable_sort(order.begin(), order.end(), [&](int c1, int c2) {
            if (lam[(size_t)c1] != lam[(size_t)c2]) return lam[(size_t)c1] > lam[(size_t)c2];  // the worst first
            return rho[(size_t)c1] < rho[(size_t)c2];
        });
        const int c = order[(size_t)j], ho = h[(size_t)c], i = c / N, jc = c % N;
        const int* row = A.data() + (size_t)c * N;
        int k = -1;
        if (q->move == MCQ_EO_MOVE_BEST) {
            int ba = INT_MAX, br = INT_MAX;
            for (int kk = 0; kk < N; kk++) {
                if (kk == ho) continue;
                const int r = (kk - oh + N) % N;
                if (row[kk] < ba || (row[kk] == ba && r < br)) ba = row[kk], br = r, k = kk;
            }
        } else {
            k = kr + (kr >= ho);
        }
        const int delta = row[k] - row[ho];
        moves++;
        uphill += delta > 0;
        flat += delta == 0;
        free_moves += row[ho] == 0;
        for (int c2 = 0; c2 < Q; c2++) {  // the rows of the aligned columns follow
            const int di = c2 / N - i, dj = c2 % N - jc, adi = di < 0 ? -di : di, adj = dj < 0 ? -dj : dj;
            if (c2 == c || !(di == 0 || dj == 0 || adi == adj)) continue;
            const int d = adi > adj ? adi : adj;
            int* row2 = A.data() + (size_t)c2 * N;
            for (int s = -1; s <= 1; s++) {
                if (ho + s * d >= 0 && ho + s * d < N) row2[ho + s * d]--;
                if (k + s * d >= 0 && k + s * d < N) row2[k + s * d]++;
            }
        }
        h[(size_t)c] = (uint8_t)k;
        E += delta;
        if (E < B) B = E, best_iter = t + 1, best = h;
        if (hist) hist[t + 1] = E;
    }
    uint8_t* out = q->state_out + ch * Q;
    for (int c = 0; c < Q; c++) out[c] = h[(size_t)c];
    if (q->best_state)
        for (int c = 0; c < Q; c++) q->best_state[ch * Q + c] = best[(size_t)c];
    store_eo_figures(*q, ch, e_in, E, B, best_iter, moves, uphill, flat, free_moves, idle);
}

}  // namespace

extern "C" {

const char* mcq_eo_last_error(void) { return g_eo_err; }

int mcq_eo_host(const mcq_eo* q) {
    const int rc = check_eo(q);
    if (rc != MCQ_OK) return rc;
    for (int i = 1; i < q->n_ranks; i++)
        if (q->rank_cdf[i] < q->rank_cdf[i - 1])
            return fail(g_eo_err, MCQ_EINVAL, "rank_cdf must not decrease: entry %d is %u behind %u", i, (unsigned)q->rank_cdf[i], (unsigned)q->rank_cdf[i - 1]);
    mcq_post::for_chains((long long)q->n_chains, [q](long long first, long long last) {
        for (long long ch = first; ch < last; ch++) host_chain(q, ch);
    });
    return MCQ_OK;
}

int mcq_eo_device(const mcq_eo* q, void* hip_stream) {
    const int rc = check_eo(q);
    if (rc != MCQ_OK) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    const EoArgs a{q->seeds, q->rank_cdf, q->state_in, q->state_out, q->best_floor, q->energy_in, q->energy_out, q->best_energy, q->best_iter,
                   q->best_state, q->n_moves, q->n_uphill, q->n_flat, q->n_free, q->n_idle, q->energy_hist, (long long)q->hist_stride,
                   (long long)q->n_chains, (long long)q->n_iters, (long long)q->first_iter, (int)q->move, (int)q->n_ranks, (int)q->N};
    mcq_table::for_rows_of(q->N, [&](auto rows) {
        hipLaunchKernelGGL(mcq_eo_kernel<decltype(rows)::NP>, dim3((unsigned)a.n_chains), dim3(64), 0, s, a);
    });
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(g_eo_err, MCQ_EDEVICE, "mcq_eo_device: %s", hipGetErrorString(e));
    return MCQ_OK;
}

}  // extern "C"
