// mcq_hop.hip -- basin hopping of board placements: kick a few columns of a minimum, descend again, keep the new minimum when it is no
// worse and go back otherwise (include/mcq.h: mcq_hop, where the rule is stated).  The local search is the descent and the pair scan of
// csrc/mcq_quench_pairs.hip, over the board table that both files take from csrc/mcq_table.h; what this file adds is the loop around them,
// as one launch.
//
//   kernel  one chain per wavefront, one wavefront per workgroup, as in the pair-move quench.  LDS holds the chain's N^2 heights, the
//           heights before the kick (N^2 bytes), the WHOLE table a(c, k) (csrc/mcq_table.h, where the layout is stated) and, with pair moves,
//           the two words per column of the scan.  The table is built ONCE per launch; every later change of a height -- a kick, a descent
//           move, a pair move, a restore -- goes through `apply`, which touches at most 6 entries in each of the <= 4 (N - 1) aligned
//           columns, one lane per aligned column.  So the table is exact behind every change, and a hop costs a handful of rows.
//           KICK: the Philox block is computed from values that are uniform over the wavefront; one block yields two (c, k) draws.
//           The draws are applied one after the other, so a column drawn twice ends on the later height.
//           RESTORE: on a rejected hop the columns are walked 64 at a time; a ballot of h[c] != saved[c] finds the columns the kick
//           and the local search changed, and `apply` puts the saved height back.  An accepted hop copies the heights over.
//           best_state goes to global memory behind the first local search and when a hop improves.
//   host    mcq_hop_host: the same rule over host buffers with plain loops; it recounts a(c, k) per use and keeps no table.
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

thread_local char g_hop_err[256] = "";

constexpr uint32_t HOP_KEY_WORD = 5u;  // key word 1 of the chain's Philox stream: 0 - 4 are the sweep's, the heat baths' and the tempered sweeps'

struct HopArgs {
    const uint32_t* seeds;
    const uint8_t* state_in;
    uint8_t* state_out;
    int32_t* energy_in;
    int32_t* energy_start;
    int32_t* energy_out;
    int32_t* best_energy;
    int64_t* best_hop;
    uint8_t* best_state;
    int64_t* n_accepted;
    int64_t* n_improved;
    int64_t* n_moves;
    int64_t* n_pair_moves;
    int32_t* energy_hist;
    long long hist_stride;
    long long n_chains;
    long long n_hops;
    long long first_hop;
    int kick;
    int slack;
    int N;
};

// the per-chain figures, by one lane or by the host: `a` is the kernel's argument struct or the parameter block
template <class A>
__host__ __device__ __forceinline__ void store_hop_figures(const A& a, long long ch, int e_in, int e_start, int E, int best, long long best_hop,
                                                           long long accepted, long long improved, long long moves, long long pair_moves) {
    if (a.energy_in) a.energy_in[ch] = e_in;
    if (a.energy_start) a.energy_start[ch] = e_start;
    if (a.energy_out) a.energy_out[ch] = E;
    if (a.best_energy) a.best_energy[ch] = best;
    if (a.best_hop) a.best_hop[ch] = best_hop;
    if (a.n_accepted) a.n_accepted[ch] = accepted;
    if (a.n_improved) a.n_improved[ch] = improved;
    if (a.n_moves) a.n_moves[ch] = moves;
    if (a.n_pair_moves) a.n_pair_moves[ch] = pair_moves;
}

// draw q of the kick of hop g: words 2 (g m + q) and 2 (g m + q) + 1 of the chain's stream, as (c, k).  `lo` and `hi` hold the two halves
// of the block of the draw before (a block serves two draws) as 64-bit words -- scalars, not an array, so that picking a half is a
// select and nothing goes to scratch --; `fresh` says that they do not.
__host__ __device__ __forceinline__ void kick_draw(uint32_t seed, unsigned long long g, int m, int q, int N, bool fresh, unsigned long long& lo,
                                                   unsigned long long& hi, int& c, int& k) {
    const unsigned long long w = 2ull * (g * (unsigned long long)m + (unsigned long long)q);
    if (fresh || (w & 3) == 0) {
        uint32_t r[4];
        philox_block((uint32_t)(w >> 2), (uint32_t)(w >> 34), seed, HOP_KEY_WORD, r);
        lo = (unsigned long long)r[0] | ((unsigned long long)r[1] << 32);
        hi = (unsigned long long)r[2] | ((unsigned long long)r[3] << 32);
    }
    const unsigned long long x = (w & 2) != 0 ? hi : lo;
    c = (int)(((x & 0xFFFFFFFFull) * (unsigned)(N * N)) >> 32);
    k = (int)(((x >> 32) * (unsigned)N) >> 32);
}

template <int NP, bool PAIRS>
__global__ __launch_bounds__(64) void mcq_hop_kernel(HopArgs a) {
    using R = mcq_table::Rows<NP>;
    constexpr int QP = R::QP, SW = R::SW, S = R::S;
    constexpr int MQ = PAIRS ? QP : 1;
    __shared__ uint32_t tab32[QP * SW];
    __shared__ uint32_t mask0[MQ], mask1[MQ];
    __shared__ uint8_t h[QP], saved[QP];
    const uint8_t* tab = reinterpret_cast<const uint8_t*>(tab32);
    const int N = a.N, Q = N * N;
    const int lane = threadIdx.x;
    const long long ch = blockIdx.x;
    const uint32_t seed = a.seeds[ch];
    const int e_in = mcq_table::start<NP>(tab32, h, a.state_in + ch * Q, N, lane);
    int E = e_in, e_start = e_in, best = e_in;
    int lm = 0, lp = 0, e0 = e_in;  // the single and pair moves of the local search that runs, and the energy it started from
    long long moves = 0, pair_moves = 0, accepted = 0, improved = 0, best_hop = 0;

    // column c takes the height hn, and the table follows
    auto apply = [&](int c, int hn) { mcq_table::apply<NP>(tab32, h, N, lane, c, hn); };

    // passes of the single-move rule until one moves nothing
    auto descend = [&]() {
        for (;;) {
            const int moved = mcq_table::pass<NP>(tab32, h, N, lane, E);
            lm += moved;
            // (lm + lp > e0 cannot happen -- every move lowers E --: it only bounds the loop should the rule ever be broken)
            if (moved == 0 || lm + lp > e0) break;
        }
    };

    const unsigned long long m = (unsigned long long)a.kick;
    // t = -1 is the local search of the input (rule item 3); t >= 0 are the hops
    for (long long t = -1; t < a.n_hops; t++) {
        const int e_prev = E;
        if (t >= 0) {  // the kick
            const unsigned long long g = (unsigned long long)(a.first_hop + t);
            unsigned long long lo = 0, hi = 0;
            for (int q = 0; q < (int)m; q++) {
                int c, k;
                kick_draw(seed, g, (int)m, q, N, q == 0, lo, hi, c, k);
                const int ho = h[c];
                if (k != ho) {
                    E += (int)tab[c * S + k] - (int)tab[c * S + ho];
                    apply(c, k);
                }
            }
        }
        // the local search
        lm = 0, lp = 0, e0 = E;
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
        moves += lm, pair_moves += lp;

        bool keeps = true, improves = false;
        if (t < 0) {
            e_start = best = E;
            improves = true;  // best_state to begin with
        } else if (E <= e_prev + a.slack) {
            accepted++;
            if (E < best) best = E, best_hop = t + 1, improved++, improves = true;
        } else {  // back to the heights before the kick: the table follows through apply
            keeps = false;
            for (int base = 0; base < Q; base += 64) {
                const int c = base + lane;
                unsigned long long diff = __ballot(c < Q && h[c] != saved[c]);
                while (diff) {
                    const int cc = base + __ffsll(diff) - 1;
                    diff &= diff - 1;
                    apply(cc, saved[cc]);
                }
            }
            E = e_prev;
        }
        if (keeps) {  // the first local search and an accepted hop: the heights are the chain's
            for (int c = lane; c < Q; c += 64) saved[c] = h[c];
            __syncthreads();
        }
        if (improves && a.best_state) {
            uint8_t* bs = a.best_state + ch * Q;
            for (int c = lane; c < Q; c += 64) bs[c] = h[c];
        }
        if (a.energy_hist && lane == 0) a.energy_hist[ch * a.hist_stride + (t + 1)] = E;
    }

    uint8_t* out = a.state_out + ch * Q;
    for (int c = lane; c < Q; c += 64) out[c] = h[c];
    if (lane == 0) store_hop_figures(a, ch, e_in, e_start, E, best, best_hop, accepted, improved, moves, pair_moves);
}

// what both entry points refuse
int check_hop(const mcq_hop* q) {
    if (!q) return fail(g_hop_err, MCQ_EINVAL, "mcq_hop: NULL parameter block");
    if (q->mode != MCQ_MODE_BOARD) return fail(g_hop_err, MCQ_EINVAL, "mode: basin hopping runs boards only (MCQ_MODE_BOARD), got %d", (int)q->mode);
    if (q->N < MCQ_MIN_N || q->N > MCQ_MAX_N_QUENCH_PAIRS)
        return fail(g_hop_err, MCQ_EINVAL, "N out of range [%d, %d]: %d", MCQ_MIN_N, MCQ_MAX_N_QUENCH_PAIRS, (int)q->N);
    if (q->n_chains < 1 || q->n_chains > INT_MAX) return fail(g_hop_err, MCQ_EINVAL, "n_chains out of range [1, 2^31 - 1]: %lld", (long long)q->n_chains);
    if (q->n_hops < 0) return fail(g_hop_err, MCQ_EINVAL, "n_hops must be >= 0 (0 = the local search alone), got %lld", (long long)q->n_hops);
    if (q->first_hop < 0) return fail(g_hop_err, MCQ_EINVAL, "first_hop must be >= 0, got %lld", (long long)q->first_hop);
    if (q->slack < 0) return fail(g_hop_err, MCQ_EINVAL, "slack must be >= 0, got %d", (int)q->slack);
    if (q->kick < 1 || q->kick > MCQ_MAX_HOP_KICK) return fail(g_hop_err, MCQ_EINVAL, "kick out of range [1, %d]: %d", MCQ_MAX_HOP_KICK, (int)q->kick);
    const unsigned __int128 words = (unsigned __int128)2 * (unsigned)q->kick * ((unsigned __int128)q->first_hop + (unsigned __int128)q->n_hops);
    if (words >= ((unsigned __int128)1 << 63))
        return fail(g_hop_err, MCQ_EINVAL, "stream words: 2 kick (first_hop + n_hops) must stay below 2^63 (kick %d, first_hop %lld, n_hops %lld)",
                    (int)q->kick, (long long)q->first_hop, (long long)q->n_hops);
    if (q->local_search != MCQ_HOP_SINGLE && q->local_search != MCQ_HOP_PAIRS)
        return fail(g_hop_err, MCQ_EINVAL, "local_search must be MCQ_HOP_SINGLE (0) or MCQ_HOP_PAIRS (1), got %d", (int)q->local_search);
    if (!q->seeds) return fail(g_hop_err, MCQ_EINVAL, "seeds is required");
    if (!q->state_in) return fail(g_hop_err, MCQ_EINVAL, "state_in is required");
    if (!q->state_out) return fail(g_hop_err, MCQ_EINVAL, "state_out is required");
    if (q->energy_hist && q->hist_stride < q->n_hops + 1)
        return fail(g_hop_err, MCQ_EINVAL, "hist_stride must be >= n_hops + 1 = %lld, got %lld", (long long)q->n_hops + 1, (long long)q->hist_stride);
    return MCQ_OK;
}

// one chain in host code: no table is kept, a(c, k) is recounted wherever it is used
void host_chain(const mcq_hop* q, long long ch) {
    const int N = q->N, Q = N * N;
    const bool pairs = q->local_search == MCQ_HOP_PAIRS;
    std::vector<uint8_t> h((size_t)Q), saved((size_t)Q);
    std::vector<int> a((size_t)N), T((size_t)Q * N), light((size_t)Q);
    mcq_table::host_load(q->state_in + ch * Q, N, h.data());
    auto recount = [&]() { return mcq_table::host_table(h.data(), N, T.data()); };
    long long moves = 0, pair_moves = 0, accepted = 0, improved = 0, best_hop = 0;
    auto descend = [&]() {
        for (;;) {
            int running = 0;  // (the energy behind a local search is recounted, not carried along)
            const int moved = mcq_table::host_pass(h.data(), N, a.data(), running);
            moves += moved;
            if (moved == 0) break;
        }
    };
    // the scan of mcq_quench_pairs, item 3, on a single-move minimum: true when it applied a pair move
    auto pair_move = [&]() {
        const mcq_table::HostPair p = mcq_table::host_scan(h.data(), N, T.data(), light.data());
        if (p.D >= 0) return false;
        h[(size_t)p.c1] = (uint8_t)p.k1, h[(size_t)p.c2] = (uint8_t)p.k2;
        pair_moves++;
        return true;
    };
    auto local_search = [&]() {
        descend();
        if (pairs)
            while (pair_move()) descend();
        return recount();
    };

    const int e_in = recount();
    const int e_start = local_search();
    int E = e_start, best = e_start;
    saved = h;
    uint8_t* bs = q->best_state ? q->best_state + ch * Q : nullptr;
    if (bs)
        for (int c = 0; c < Q; c++) bs[c] = h[(size_t)c];
    int32_t* hist = q->energy_hist ? q->energy_hist + ch * q->hist_stride : nullptr;
    if (hist) hist[0] = E;
    const uint32_t seed = q->seeds[ch];
    for (long long t = 0; t < q->n_hops; t++) {
        unsigned long long lo = 0, hi = 0;
        for (int d = 0; d < q->kick; d++) {
            int c, k;
            kick_draw(seed, (unsigned long long)(q->first_hop + t), q->kick, d, N, d == 0, lo, hi, c, k);
            h[(size_t)c] = (uint8_t)k;
        }
        const int e_new = local_search();
        if (e_new <= E + q->slack) {
            E = e_new;
            saved = h;
            accepted++;
            if (E < best) {
                best = E, best_hop = t + 1, improved++;
                if (bs)
                    for (int c = 0; c < Q; c++) bs[c] = h[(size_t)c];
            }
        } else {
            h = saved;
        }
        if (hist) hist[t + 1] = E;
    }
    uint8_t* out = q->state_out + ch * Q;
    for (int c = 0; c < Q; c++) out[c] = h[(size_t)c];
    store_hop_figures(*q, ch, e_in, e_start, E, best, best_hop, accepted, improved, moves, pair_moves);
}

}  // namespace

extern "C" {

const char* mcq_hop_last_error(void) { return g_hop_err; }

int mcq_hop_host(const mcq_hop* q) {
    const int rc = check_hop(q);
    if (rc != MCQ_OK) return rc;
    mcq_post::for_chains((long long)q->n_chains, [q](long long first, long long last) {
        for (long long ch = first; ch < last; ch++) host_chain(q, ch);
    });
    return MCQ_OK;
}

int mcq_hop_device(const mcq_hop* q, void* hip_stream) {
    const int rc = check_hop(q);
    if (rc != MCQ_OK) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    const HopArgs a{q->seeds, q->state_in, q->state_out, q->energy_in, q->energy_start, q->energy_out, q->best_energy, q->best_hop, q->best_state,
                    q->n_accepted, q->n_improved, q->n_moves, q->n_pair_moves, q->energy_hist, (long long)q->hist_stride, (long long)q->n_chains,
                    (long long)q->n_hops, (long long)q->first_hop, (int)q->kick, (int)q->slack, (int)q->N};
    const bool pairs = q->local_search == MCQ_HOP_PAIRS;
    mcq_table::for_rows_of(q->N, [&](auto rows) {
        constexpr int NP = decltype(rows)::NP;
        if (pairs) hipLaunchKernelGGL((mcq_hop_kernel<NP, true>), dim3((unsigned)a.n_chains), dim3(64), 0, s, a);
        else hipLaunchKernelGGL((mcq_hop_kernel<NP, false>), dim3((unsigned)a.n_chains), dim3(64), 0, s, a);
    });
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(g_hop_err, MCQ_EDEVICE, "mcq_hop_device: %s", hipGetErrorString(e));
    return MCQ_OK;
}

}  // extern "C"
