// mcq_relink.hip -- path relinking between board placements: walk from a placement towards a guide, one column at a time, always the
// cheapest remaining column, and hand the best placement met on the way to the local search (include/mcq.h: mcq_relink, where the rule
// is stated).  The table a(c, k), `apply`, `pass` and `scan` are those of csrc/mcq_table.h, and the local search is the loop of
// csrc/mcq_hop.hip; what this file adds is the walk between two placements, as one launch.
//
//   kernel  one chain per wavefront, one wavefront per workgroup, as in the hops.  LDS holds the WHOLE table a(c, k) in the layout of
//           csrc/mcq_table.h, the walking heights h, the guide g and the best placement of the path (N^2 bytes each) and, with pair
//           moves, the two words per column of the scan.  The table is built ONCE per launch; every change of a height -- a step of the
//           walk, a step back, a move of the local search -- goes through `apply`.
//           STEP: the Philox block is computed from values that are uniform over the wavefront.  Each lane takes its columns 64 apart;
//           a column with h != g reads the two table bytes a(c, g(c)) and a(c, h(c)) and forms one 32-bit key
//           (delta + 128) << 10 | rho (|delta| <= 4 (N - 1) = 124, rho < N^2 <= 2^10); a __shfl_xor butterfly picks the smallest.
//           Then `apply`, E, the history, and a copy of h when the step is a candidate with a new low.
//           BACK: behind the walk the table must be that of the best placement P*.  The columns with h != P* are walked 64 at a time by
//           ballot and `apply` puts P*'s height back: at most as many applies as the walk took behind P*, each a handful of rows,
//           where a rebuild gathers all N^3 entries over 4 (N - 1) columns each (N^4 / 16 reads a lane; 65 536 at N = 32 against
//           at most 1 024 applies of two trips).
//           Then the local search of csrc/mcq_hop.hip, guards included.
//   host    mcq_relink_host: the same rule over host buffers with plain loops; a table of ints follows the steps of the walk, and the
//           local search recounts as the host code of the hops does.
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

thread_local char g_relink_err[256] = "";

constexpr uint32_t RELINK_KEY_WORD = 9u;  // key word 1 of the chain's Philox stream: 0 - 8 are taken (include/mcq.h: mcq_relink, item 2)
constexpr int DELTA_BIAS = 128;           // above 4 (MCQ_MAX_N_QUENCH_PAIRS - 1) = 124: delta + DELTA_BIAS > 0
constexpr int RHO_BITS = 10;              // rho < 32^2
constexpr uint32_t KEY_NONE = 0xFFFFFFFFu;

struct RelinkArgs {
    const uint32_t* seeds;
    const uint8_t* state_in;
    const uint8_t* guide_in;
    uint8_t* state_out;
    uint8_t* path_best_state;
    int32_t* distance_in;
    int32_t* n_steps;
    int32_t* path_best_step;
    int32_t* energy_in;
    int32_t* path_best_energy;
    int32_t* path_max_energy;
    int32_t* energy_out;
    int64_t* n_moves;
    int64_t* n_pair_moves;
    int32_t* energy_hist;
    long long hist_stride;
    long long n_chains;
    long long walk;
    int max_steps;
    int min_dist;
    int N;
};

// the per-chain figures, by one lane or by the host: `a` is the kernel's argument struct or the parameter block
template <class A>
__host__ __device__ __forceinline__ void store_relink_figures(const A& a, long long ch, int d0, int n_steps, int best_step, int e_in, int best_e,
                                                              int e_max, int E, long long moves, long long pair_moves) {
    if (a.distance_in) a.distance_in[ch] = d0;
    if (a.n_steps) a.n_steps[ch] = n_steps;
    if (a.path_best_step) a.path_best_step[ch] = best_step;
    if (a.energy_in) a.energy_in[ch] = e_in;
    if (a.path_best_energy) a.path_best_energy[ch] = best_e;
    if (a.path_max_energy) a.path_max_energy[ch] = e_max;
    if (a.energy_out) a.energy_out[ch] = E;
    if (a.n_moves) a.n_moves[ch] = moves;
    if (a.n_pair_moves) a.n_pair_moves[ch] = pair_moves;
}

// the tie offset o of step t of walk `walk`: word 0 of philox4x32-10(counter = (t, walk low, walk high, 0), key = (seed, 9))
__host__ __device__ __forceinline__ int relink_draw(uint32_t seed, uint32_t t, unsigned long long walk, int Q) {
    uint32_t c0 = t, c1 = (uint32_t)walk, c2 = (uint32_t)(walk >> 32), c3 = 0, k0 = seed, k1 = RELINK_KEY_WORD;
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1, c3 = (uint32_t)p0, c0 = n0, c2 = n2;
        k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
    }
    return (int)(((unsigned long long)c0 * (unsigned)Q) >> 32);
}

// whether the placement behind step t (counted from 1) is a candidate: rule item 3
__host__ __device__ __forceinline__ bool is_candidate(int t, int d0, int min_dist) { return t >= (min_dist > 1 ? min_dist : 1) && d0 - t >= min_dist; }

template <int NP, bool PAIRS>
constexpr int relink_lds_bytes() {
    return NP * NP * (4 * ((NP / 4) | 1) + 3) + (PAIRS ? 8 * NP * NP : 0);
}

template <int NP, bool PAIRS>
__global__ __launch_bounds__(64) void mcq_relink_kernel(RelinkArgs a) {
    using R = mcq_table::Rows<NP>;
    constexpr int QP = R::QP, SW = R::SW, S = R::S;
    constexpr int MQ = PAIRS ? QP : 1;
    __shared__ uint32_t tab32[QP * SW];
    __shared__ uint32_t mask0[MQ], mask1[MQ];
    __shared__ uint8_t h[QP], g[QP], pbest[QP];
    // (without pair moves the two mask words are never touched and take no LDS)
    static_assert(sizeof(tab32) + (PAIRS ? sizeof(mask0) + sizeof(mask1) : 0) + sizeof(h) + sizeof(g) + sizeof(pbest) == relink_lds_bytes<NP, PAIRS>(),
                  "the LDS of a chain, as the host checks it");
    static_assert(relink_lds_bytes<NP, PAIRS>() <= MCQ_MAX_RELINK_LDS, "a chain fits the LDS of a workgroup");
    const uint8_t* tab = reinterpret_cast<const uint8_t*>(tab32);
    const int N = a.N, Q = N * N;
    const int lane = threadIdx.x;
    const long long ch = blockIdx.x;
    const uint32_t seed = a.seeds[ch];
    const uint8_t* in = a.state_in + ch * Q;
    const uint8_t* gin = a.guide_in + ch * Q;
    int d0 = 0;
    for (int base = 0; base < Q; base += 64) {
        const int c = base + lane;
        bool differs = false;
        if (c < Q) {
            const uint8_t hc = mcq_table::clamped(in[c], N), gc = mcq_table::clamped(gin[c], N);
            h[c] = hc, g[c] = gc, pbest[c] = hc;
            differs = hc != gc;
        }
        d0 += __popcll(__ballot(differs));
    }
    mcq_table::fill<NP>(tab32, Q, lane);
    __syncthreads();
    mcq_table::build<NP>(tab32, h, N, lane);
    const int e_in = mcq_table::energy<NP>(tab32, h, N, lane);
    int E = e_in, e_max = e_in, best_e = INT_MAX, best_step = 0;
    const int n_steps = a.max_steps == 0 ? d0 : min(d0, a.max_steps);
    const int W = a.max_steps == 0 ? Q : a.max_steps;
    int32_t* hist = a.energy_hist ? a.energy_hist + ch * a.hist_stride : nullptr;
    if (hist && lane == 0) hist[0] = E;

    auto apply = [&](int c, int hn) { mcq_table::apply<NP>(tab32, h, N, lane, c, hn); };

    // the walk
    for (int t = 0; t < n_steps; t++) {
        const int o = relink_draw(seed, (uint32_t)t, (unsigned long long)a.walk, Q);
        uint32_t key = KEY_NONE;
        for (int c = lane; c < Q; c += 64) {
            const int hc = h[c], gc = g[c];
            if (hc == gc) continue;
            const int delta = (int)tab[c * S + gc] - (int)tab[c * S + hc];
            int rho = c - o;
            rho += rho < 0 ? Q : 0;
            key = min(key, ((uint32_t)(delta + DELTA_BIAS) << RHO_BITS) | (uint32_t)rho);
        }
        for (int x = 32; x; x >>= 1) key = min(key, (uint32_t)__shfl_xor((int)key, x));
        if (key == KEY_NONE) break;  // (cannot happen -- n_steps <= d0 columns differ --: it only keeps a broken rule inside the arrays)
        int c = (int)(key & ((1u << RHO_BITS) - 1u)) + o;
        c -= c >= Q ? Q : 0;
        E += (int)(key >> RHO_BITS) - DELTA_BIAS;
        apply(c, g[c]);
        e_max = max(e_max, E);
        if (is_candidate(t + 1, d0, a.min_dist) && E < best_e) {
            best_e = E, best_step = t + 1;
            for (int cc = lane; cc < Q; cc += 64) pbest[cc] = h[cc];
            __syncthreads();
        }
        if (hist && lane == 0) hist[t + 1] = E;
    }
    if (hist)
        for (int t = n_steps + 1 + lane; t <= W; t += 64) hist[t] = E;
    if (best_step == 0) best_e = e_in;  // no candidate: P* is the clamped input, which pbest still holds

    // back to P*: the table follows through apply
    for (int base = 0; base < Q; base += 64) {
        const int c = base + lane;
        unsigned long long diff = __ballot(c < Q && h[c] != pbest[c]);
        while (diff) {
            const int cc = base + __ffsll(diff) - 1;
            diff &= diff - 1;
            apply(cc, pbest[cc]);
        }
    }
    E = best_e;

    // the local search of csrc/mcq_hop.hip on P*
    int lm = 0, lp = 0;
    const int e0 = E;
    auto descend = [&]() {
        for (;;) {
            const int moved = mcq_table::pass<NP>(tab32, h, N, lane, E);
            lm += moved;
            // (lm + lp > e0 cannot happen -- every move lowers E --: it only bounds the loop should the rule ever be broken)
            if (moved == 0 || lm + lp > e0) break;
        }
    };
    descend();
    if constexpr (PAIRS) {
        for (;;) {
            const unsigned long long key = mcq_table::scan<NP>(tab32, h, mask0, mask1, N, lane);
            if (key >= mcq_table::PAIR_KEY_NONE) break;
            const int D = (int)(key >> 40) - 4;
            apply((int)(key >> 30) & 1023, (int)(key >> 10) & 1023);
            apply((int)(key >> 20) & 1023, (int)key & 1023);
            E += D;
            lp++;
            descend();
            if (lm + lp > e0) break;
        }
    }

    uint8_t* out = a.state_out + ch * Q;
    for (int c = lane; c < Q; c += 64) out[c] = h[c];
    if (a.path_best_state) {
        uint8_t* bs = a.path_best_state + ch * Q;
        for (int c = lane; c < Q; c += 64) bs[c] = pbest[c];
    }
    if (lane == 0) store_relink_figures(a, ch, d0, n_steps, best_step, e_in, best_e, e_max, E, (long long)lm, (long long)lp);
}

int lds_bytes(int N, bool pairs) {
    return mcq_table::for_rows_of(N, [pairs](auto rows) {
        constexpr int NP = decltype(rows)::NP;
        return pairs ? relink_lds_bytes<NP, true>() : relink_lds_bytes<NP, false>();
    });
}

// W of rule item 5: the last entry of a chain's history
long long hist_width(const mcq_relink* q) { return q->max_steps == 0 ? (long long)q->N * q->N : (long long)q->max_steps; }

// what both entry points refuse
int check_relink(const mcq_relink* q) {
    if (!q) return fail(g_relink_err, MCQ_EINVAL, "mcq_relink: NULL parameter block");
    if (q->mode != MCQ_MODE_BOARD) return fail(g_relink_err, MCQ_EINVAL, "mode: path relinking runs boards only (MCQ_MODE_BOARD), got %d", (int)q->mode);
    if (q->N < MCQ_MIN_N || q->N > MCQ_MAX_N_QUENCH_PAIRS)
        return fail(g_relink_err, MCQ_EINVAL, "N out of range [%d, %d]: %d", MCQ_MIN_N, MCQ_MAX_N_QUENCH_PAIRS, (int)q->N);
    if (q->n_chains < 1 || q->n_chains > INT_MAX) return fail(g_relink_err, MCQ_EINVAL, "n_chains out of range [1, 2^31 - 1]: %lld", (long long)q->n_chains);
    const int Q = q->N * q->N;
    if (q->max_steps < 0 || q->max_steps > Q)
        return fail(g_relink_err, MCQ_EINVAL, "max_steps out of range [0, N^2 = %d] (0 = the whole way to the guide): %d", Q, (int)q->max_steps);
    if (q->min_dist < 0 || q->min_dist > Q) return fail(g_relink_err, MCQ_EINVAL, "min_dist out of range [0, N^2 = %d]: %d", Q, (int)q->min_dist);
    if (q->local_search != MCQ_HOP_SINGLE && q->local_search != MCQ_HOP_PAIRS)
        return fail(g_relink_err, MCQ_EINVAL, "local_search must be MCQ_HOP_SINGLE (0) or MCQ_HOP_PAIRS (1), got %d", (int)q->local_search);
    if (q->walk < 0) return fail(g_relink_err, MCQ_EINVAL, "walk must be >= 0, got %lld", (long long)q->walk);
    if (!q->seeds) return fail(g_relink_err, MCQ_EINVAL, "seeds is required");
    if (!q->state_in) return fail(g_relink_err, MCQ_EINVAL, "state_in is required");
    if (!q->guide_in) return fail(g_relink_err, MCQ_EINVAL, "guide_in is required");
    if (!q->state_out) return fail(g_relink_err, MCQ_EINVAL, "state_out is required");
    if (q->state_out == q->guide_in) return fail(g_relink_err, MCQ_EINVAL, "state_out must be distinct from guide_in (it may be state_in)");
    if (q->path_best_state && (q->path_best_state == q->state_in || q->path_best_state == q->guide_in || q->path_best_state == q->state_out))
        return fail(g_relink_err, MCQ_EINVAL, "path_best_state must be distinct from state_in, guide_in and state_out");
    if (q->energy_hist && q->hist_stride < hist_width(q) + 1)
        return fail(g_relink_err, MCQ_EINVAL, "hist_stride must be >= W + 1 = %lld (W = max_steps, or N^2 when that is 0), got %lld", hist_width(q) + 1,
                    (long long)q->hist_stride);
    const int lds = lds_bytes(q->N, q->local_search == MCQ_HOP_PAIRS);
    if (lds > MCQ_MAX_RELINK_LDS)
        return fail(g_relink_err, MCQ_EINVAL, "N = %d: a chain takes %d bytes of LDS, above the %d of a workgroup", (int)q->N, lds, MCQ_MAX_RELINK_LDS);
    return MCQ_OK;
}

// one chain in host code: a table of ints follows the steps of the walk; the local search recounts a(c, k) wherever it is used
void host_chain(const mcq_relink* q, long long ch) {
    const int N = q->N, Q = N * N;
    const bool pairs = q->local_search == MCQ_HOP_PAIRS;
    std::vector<uint8_t> h((size_t)Q), g((size_t)Q), pbest;
    std::vector<int> a((size_t)N), T((size_t)Q * N), light((size_t)Q);
    mcq_table::host_load(q->state_in + ch * Q, N, h.data());
    mcq_table::host_load(q->guide_in + ch * Q, N, g.data());
    pbest = h;
    const uint32_t seed = q->seeds[ch];
    const int e_in = mcq_table::host_table(h.data(), N, T.data());
    int d0 = 0;
    for (int c = 0; c < Q; c++) d0 += h[(size_t)c] != g[(size_t)c];
    const int n_steps = q->max_steps == 0 ? d0 : (d0 < q->max_steps ? d0 : q->max_steps);
    const long long W = hist_width(q);
    int32_t* hist = q->energy_hist ? q->energy_hist + ch * q->hist_stride : nullptr;
    int E = e_in, e_max = e_in, best_e = INT_MAX, best_step = 0;
    if (hist) hist[0] = E;
    for (int t = 0; t < n_steps; t++) {
        const int o = relink_draw(seed, (uint32_t)t, (unsigned long long)q->walk, Q);
        int bd = INT_MAX, brho = INT_MAX, bc = -1;
        for (int c = 0; c < Q; c++) {
            if (h[(size_t)c] == g[(size_t)c]) continue;
            const int delta = T[(size_t)c * N + g[(size_t)c]] - T[(size_t)c * N + h[(size_t)c]];
            const int rho = (c - o + Q) % Q;
            if (delta < bd || (delta == bd && rho < brho)) bd = delta, brho = rho, bc = c;
        }
        const int ho = h[(size_t)bc], hn = g[(size_t)bc], i = bc / N, j = bc % N;
        for (int c2 = 0; c2 < Q; c2++) {  // the rows of the aligned columns follow
            const int di = c2 / N - i, dj = c2 % N - j, adi = di < 0 ? -di : di, adj = dj < 0 ? -dj : dj;
            if (c2 == bc || !(di == 0 || dj == 0 || adi == adj)) continue;
            const int d = adi > adj ? adi : adj;
            int* row = T.data() + (size_t)c2 * N;
            for (int s = -1; s <= 1; s++) {
                if (ho + s * d >= 0 && ho + s * d < N) row[ho + s * d]--;
                if (hn + s * d >= 0 && hn + s * d < N) row[hn + s * d]++;
            }
        }
        h[(size_t)bc] = (uint8_t)hn;
        E += bd;
        if (E > e_max) e_max = E;
        if (is_candidate(t + 1, d0, q->min_dist) && E < best_e) best_e = E, best_step = t + 1, pbest = h;
        if (hist) hist[t + 1] = E;
    }
    if (hist)
        for (long long t = n_steps + 1; t <= W; t++) hist[t] = E;
    if (best_step == 0) best_e = e_in;

    // the local search on P*, as the host code of the hops runs it
    h = pbest;
    long long moves = 0, pair_moves = 0;
    auto descend = [&]() {
        for (;;) {
            int running = 0;  // (the energy behind the local search is recounted, not carried along)
            const int moved = mcq_table::host_pass(h.data(), N, a.data(), running);
            moves += moved;
            if (moved == 0) break;
        }
    };
    descend();
    if (pairs)
        for (;;) {
            const mcq_table::HostPair p = mcq_table::host_scan(h.data(), N, T.data(), light.data());
            if (p.D >= 0) break;
            h[(size_t)p.c1] = (uint8_t)p.k1, h[(size_t)p.c2] = (uint8_t)p.k2;
            pair_moves++;
            descend();
        }
    E = mcq_table::host_table(h.data(), N, T.data());

    uint8_t* out = q->state_out + ch * Q;
    for (int c = 0; c < Q; c++) out[c] = h[(size_t)c];
    if (q->path_best_state)
        for (int c = 0; c < Q; c++) q->path_best_state[ch * Q + c] = pbest[(size_t)c];
    store_relink_figures(*q, ch, d0, n_steps, best_step, e_in, best_e, e_max, E, moves, pair_moves);
}

}  // namespace

extern "C" {

const char* mcq_relink_last_error(void) { return g_relink_err; }

int mcq_relink_host(const mcq_relink* q) {
    const int rc = check_relink(q);
    if (rc != MCQ_OK) return rc;
    mcq_post::for_chains((long long)q->n_chains, [q](long long first, long long last) {
        for (long long ch = first; ch < last; ch++) host_chain(q, ch);
    });
    return MCQ_OK;
}

int mcq_relink_device(const mcq_relink* q, void* hip_stream) {
    const int rc = check_relink(q);
    if (rc != MCQ_OK) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    const RelinkArgs a{q->seeds, q->state_in, q->guide_in, q->state_out, q->path_best_state, q->distance_in, q->n_steps, q->path_best_step,
                       q->energy_in, q->path_best_energy, q->path_max_energy, q->energy_out, q->n_moves, q->n_pair_moves, q->energy_hist,
                       (long long)q->hist_stride, (long long)q->n_chains, (long long)q->walk, (int)q->max_steps, (int)q->min_dist, (int)q->N};
    const bool pairs = q->local_search == MCQ_HOP_PAIRS;
    mcq_table::for_rows_of(q->N, [&](auto rows) {
        constexpr int NP = decltype(rows)::NP;
        if (pairs) hipLaunchKernelGGL((mcq_relink_kernel<NP, true>), dim3((unsigned)a.n_chains), dim3(64), 0, s, a);
        else hipLaunchKernelGGL((mcq_relink_kernel<NP, false>), dim3((unsigned)a.n_chains), dim3(64), 0, s, a);
    });
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(g_relink_err, MCQ_EDEVICE, "mcq_relink_device: %s", hipGetErrorString(e));
    return MCQ_OK;
}

}  // extern "C"
