// mcq_hop.hip -- basin hopping of board placements: kick a few columns of a minimum, descend again, keep the new minimum when it is no
// worse and go back otherwise (include/mcq.h: mcq_hop, where the rule is stated).  The local search is the descent and the pair scan of
// csrc/mcq_quench_pairs.hip, restated here so that file stays as it is; what this file adds is the loop around them, as one launch.
//
//   kernel  one chain per wavefront, one wavefront per workgroup, as in the pair-move quench.  LDS holds the chain's N^2 heights, the
//           heights before the kick (N^2 bytes), the WHOLE table a(c, k) as one byte per entry in rows of S bytes (S a multiple of 4
//           with an odd number of dwords: a lane per column reads its row as dwords without bank conflicts) and, with pair moves, the
//           two words per column of the scan.  The table is built ONCE per launch; every later change of a height -- a kick, a descent
//           move, a pair move, a restore -- goes through `apply`, which touches at most 6 entries in each of the <= 4 (N - 1) aligned
//           columns, one lane per aligned column.  So the table is exact behind every change, and a hop costs a handful of rows.
//           KICK: the Philox block is computed from values that are uniform over the wavefront; one block yields two (c, k) draws.
//           The draws are applied one after the other, so a column drawn twice ends on the later height.
//           RESTORE: on a rejected hop the columns are walked 64 at a time; a ballot of h[c] != saved[c] finds the columns the kick
//           and the local search changed, and `apply` puts the saved height back.  An accepted hop copies the heights over.
//           Every data-dependent loop is uniform over the wavefront (one chain), so __syncthreads() is legal wherever lanes hand LDS
//           data to each other; in a workgroup of one wavefront it is no hardware barrier, only the wait for the LDS counter and a
//           fence for the compiler.  best_state goes to global memory behind the first local search and when a hop improves.
//   host    mcq_hop_host: the same rule over host buffers with plain loops; it recounts a(c, k) per use and keeps no table.
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

__host__ __device__ __forceinline__ int att(int k, int kk, int d) {
    const int x = k > kk ? k - kk : kk - k;
    return (x == 0) | (x == d);
}

// the scan's key: D + 4 above c1, c2, k1, k2 (10 bits each), so that the smallest key is the lexicographically smallest candidate
constexpr unsigned long long KEY_NONE = 4ull << 40;  // D = 0: no candidate improves
__device__ __forceinline__ unsigned long long pack_key(int D, int c1, int c2, int k1, int k2) {
    return ((unsigned long long)(D + 4) << 40) | ((unsigned long long)c1 << 30) | ((unsigned long long)c2 << 20) | ((unsigned long long)k1 << 10) | (unsigned long long)k2;
}

// slot t = 0 .. 4 N - 1 of column (i, j): position p = t mod N of its row, its board column, its diagonal, its antidiagonal.  True when
// the slot names another column of the board, c2, at distance d; every aligned column has exactly one slot.
__device__ __forceinline__ bool aligned_slot(int N, int i, int j, int t, int& c2, int& d) {
    const int f = (t >= N) + (t >= 2 * N) + (t >= 3 * N), p = t - f * N;
    const int off = p - (f == 1 ? i : j);
    d = off < 0 ? -off : off;
    const int r = f == 0 ? i : f == 1 ? p : f == 2 ? i + off : i - off;
    c2 = r * N + (f == 1 ? j : p);
    return t < 4 * N && off != 0 && r >= 0 && r < N;
}

template <int NP, bool PAIRS>
__global__ __launch_bounds__(64) void mcq_hop_kernel(HopArgs a) {
    constexpr int QP = NP * NP;
    constexpr int SW = (NP / 4) | 1, S = 4 * SW;  // dwords and bytes of a table row
    constexpr int RW = NP / 4;                    // dwords of a row that hold entries
    constexpr int MQ = PAIRS ? QP : 1;
    __shared__ uint32_t tab32[QP * SW];
    __shared__ uint32_t mask0[MQ], mask1[MQ];
    __shared__ uint8_t h[QP], saved[QP];
    uint8_t* tab = reinterpret_cast<uint8_t*>(tab32);
    const int N = a.N, Q = N * N;
    const int lane = threadIdx.x;
    const long long ch = blockIdx.x;
    const uint32_t seed = a.seeds[ch];
    const uint8_t* in = a.state_in + ch * Q;
    for (int c = lane; c < Q; c += 64) {
        const int v = in[c];
        h[c] = (uint8_t)(v < N ? v : N - 1);
    }
    for (int w = lane; w < Q * SW; w += 64) tab32[w] = 0xFFFFFFFFu;  // what lies behind k = N - 1 never wins an argmin
    __syncthreads();
    for (int e = lane; e < Q * N; e += 64) {  // the table, one lane per entry
        const int c = e / N, k = e - c * N, i = c / N, j = c - i * N;
        int cnt = 0;
        auto hit = [&](int hp, int d) { cnt += att(hp, k, d); };
        for (int jj = 0; jj < N; jj++) {  // the row, and the two diagonal cells of board column jj
            if (jj == j) continue;
            const int d = jj > j ? jj - j : j - jj;
            hit(h[i * N + jj], d);
            if (i + d < N) hit(h[(i + d) * N + jj], d);
            if (i - d >= 0) hit(h[(i - d) * N + jj], d);
        }
        for (int ii = 0; ii < N; ii++)  // the board column
            if (ii != i) hit(h[ii * N + j], ii > i ? ii - i : i - ii);
        tab[c * S + k] = (uint8_t)cnt;
    }
    __syncthreads();

    int twoE = 0;
    for (int c = lane; c < Q; c += 64) twoE += tab[c * S + h[c]];
    for (int o = 32; o; o >>= 1) twoE += __shfl_xor(twoE, o);
    const int e_in = twoE >> 1;
    int E = e_in, e_start = e_in, best = e_in;
    int lm = 0, lp = 0, e0 = e_in;  // the single and pair moves of the local search that runs, and the energy it started from
    long long moves = 0, pair_moves = 0, accepted = 0, improved = 0, best_hop = 0;

    // column c takes the height hn: the table rows of its aligned columns follow, one lane per aligned column
    auto apply = [&](int c, int hn) {
        const int i = c / N, j = c - i * N, ho = h[c];
        for (int t = lane; t < 4 * N; t += 64) {
            int c2, d;
            if (!aligned_slot(N, i, j, t, c2, d)) continue;
            uint8_t* row = tab + c2 * S;
            row[ho]--;
            if (ho - d >= 0) row[ho - d]--;
            if (ho + d < N) row[ho + d]--;
            row[hn]++;
            if (hn - d >= 0) row[hn - d]++;
            if (hn + d < N) row[hn + d]++;
        }
        h[c] = (uint8_t)hn;
        __syncthreads();
    };

    // passes of the single-move rule until one moves nothing
    auto descend = [&]() {
        for (;;) {
            int moved = 0;
            for (int cur = 0; cur < Q;) {
                const int c = cur + lane;
                int key = INT_MAX, now = 0;
                if (c < Q) {
                    const uint32_t* row = tab32 + c * SW;
#pragma unroll
                    for (int w = 0; w < RW; w++) {
                        const uint32_t v = row[w];
#pragma unroll
                        for (int b = 0; b < 4; b++) key = min(key, (int)((((v >> (8 * b)) & 255u) << 8) | (uint32_t)(4 * w + b)));
                    }
                    now = tab[c * S + h[c]];
                }
                const unsigned long long improving = __ballot(c < Q && (key >> 8) < now);
                if (!improving) {
                    cur += 64;
                    continue;
                }
                const int first = __ffsll(improving) - 1;
                const int kbest = __shfl(key, first) & 255, drop = __shfl(now - (key >> 8), first);
                E -= drop;
                moved++;
                apply(cur + first, kbest);
                cur += first + 1;
            }
            lm += moved;
            // (lm + lp > e0 cannot happen -- every move lowers E --: it only bounds the loop should the rule ever be broken)
            if (moved == 0 || lm + lp > e0) break;
        }
    };

    // the smallest key over the aligned pairs; KEY_NONE or above when no pair improves
    auto scan = [&]() {
        for (int c = lane; c < Q; c += 64) {
            const int hc = h[c], now = tab[c * S + hc];
            const uint32_t* row = tab32 + c * SW;
            uint32_t m0 = 0, m1 = 0;
#pragma unroll
            for (int w = 0; w < RW; w++) {
                const uint32_t v = row[w];
#pragma unroll
                for (int b = 0; b < 4; b++) {
                    const int dl = (int)((v >> (8 * b)) & 255u) - now;
                    m0 |= (uint32_t)(dl == 0) << (4 * w + b);
                    m1 |= (uint32_t)(dl == 1) << (4 * w + b);
                }
            }
            mask0[c] = m0 & ~(1u << hc);
            mask1[c] = m1;
        }
        __syncthreads();
        unsigned long long key = ~0ull;
        for (int base = 0; base < Q; base += 64) {
            const int c = base + lane;
            unsigned long long live = __ballot(c < Q && (mask0[c] | mask1[c]) != 0);
            while (live) {
                const int c1 = base + __ffsll(live) - 1;
                live &= live - 1;
                const int i = c1 / N, j = c1 - i * N, h1 = h[c1];
                const uint32_t a0 = mask0[c1], a1 = mask1[c1];
                for (int t = lane; t < 4 * N; t += 64) {
                    int c2, d;
                    if (!aligned_slot(N, i, j, t, c2, d) || c2 <= c1) continue;
                    const uint32_t b0 = mask0[c2], b1 = mask1[c2];
                    if (!(b0 | b1)) continue;
                    const int h2 = h[c2], hh = att(h1, h2, d);
                    for (uint32_t m = a0 | a1; m; m &= m - 1) {
                        const int k1 = __builtin_ctz(m), d1 = (int)((a1 >> k1) & 1u), kh = att(k1, h2, d);
                        for (uint32_t n = d1 ? b0 : (b0 | b1); n; n &= n - 1) {
                            const int k2 = __builtin_ctz(n), d2 = (int)((b1 >> k2) & 1u);
                            const int D = d1 + d2 - kh - att(h1, k2, d) + hh + att(k1, k2, d);
                            if (D < 0) key = min(key, pack_key(D, c1, c2, k1, k2));
                        }
                    }
                }
            }
        }
        for (int o = 32; o; o >>= 1) key = min(key, __shfl_xor(key, o));
        return key;
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
                const unsigned long long key = scan();
                if (key >= KEY_NONE) break;
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

template <int NP>
void launch_hop(const HopArgs& a, bool pairs, hipStream_t s) {
    if (pairs) hipLaunchKernelGGL((mcq_hop_kernel<NP, true>), dim3((unsigned)a.n_chains), dim3(64), 0, s, a);
    else hipLaunchKernelGGL((mcq_hop_kernel<NP, false>), dim3((unsigned)a.n_chains), dim3(64), 0, s, a);
}

// one chain in host code: no table is kept, a(c, k) is recounted wherever it is used
void host_chain(const mcq_hop* q, long long ch) {
    const int N = q->N, Q = N * N;
    const bool pairs = q->local_search == MCQ_HOP_PAIRS;
    std::vector<uint8_t> h((size_t)Q), saved((size_t)Q);
    std::vector<int> a((size_t)N), T((size_t)Q * N), light((size_t)Q);
    const uint8_t* in = q->state_in + ch * Q;
    for (int c = 0; c < Q; c++) h[(size_t)c] = (uint8_t)(in[c] < N ? in[c] : N - 1);
    auto recount = [&]() {
        long long twoE = 0;
        for (int c = 0; c < Q; c++) {
            host_counts(h.data(), N, c / N, c % N, a.data());
            twoE += a[h[(size_t)c]];
        }
        return (int)(twoE / 2);
    };
    long long moves = 0, pair_moves = 0, accepted = 0, improved = 0, best_hop = 0;
    auto descend = [&]() {
        for (;;) {
            int moved = 0;
            for (int c = 0; c < Q; c++) {
                host_counts(h.data(), N, c / N, c % N, a.data());
                int best = 0;
                for (int k = 1; k < N; k++)
                    if (a[k] < a[best]) best = k;  // strictly: the smallest k of the minimum
                if (a[best] < a[h[(size_t)c]]) {
                    h[(size_t)c] = (uint8_t)best;
                    moved++;
                }
            }
            moves += moved;
            if (moved == 0) break;
        }
    };
    // the scan of mcq_quench_pairs, item 3, on a single-move minimum: true when it applied a pair move
    auto pair_move = [&]() {
        for (int c = 0; c < Q; c++) {
            host_counts(h.data(), N, c / N, c % N, T.data() + (size_t)c * N);
            const int* row = T.data() + (size_t)c * N;
            light[(size_t)c] = 0;  // a column without a height k != h of difference <= 1 is in no improving pair
            for (int k = 0; k < N; k++)
                if (k != h[(size_t)c] && row[k] - row[h[(size_t)c]] <= 1) light[(size_t)c] = 1;
        }
        int bD = 0, b1 = -1, b2 = -1, bk1 = -1, bk2 = -1;
        for (int c1 = 0; c1 < Q; c1++) {
            if (!light[(size_t)c1]) continue;
            const int i1 = c1 / N, j1 = c1 % N, h1 = h[(size_t)c1];
            const int* r1 = T.data() + (size_t)c1 * N;
            for (int c2 = c1 + 1; c2 < Q; c2++) {
                if (!light[(size_t)c2]) continue;
                const int di = c2 / N - i1, dj = c2 % N - j1, adi = di < 0 ? -di : di, adj = dj < 0 ? -dj : dj;
                if (!(di == 0 || dj == 0 || adi == adj)) continue;
                const int d = adi > adj ? adi : adj, h2 = h[(size_t)c2];
                const int* r2 = T.data() + (size_t)c2 * N;
                for (int k1 = 0; k1 < N; k1++) {
                    const int d1 = r1[k1] - r1[h1];
                    if (k1 == h1 || d1 > 1) continue;
                    for (int k2 = 0; k2 < N; k2++) {
                        const int d2 = r2[k2] - r2[h2];
                        if (k2 == h2 || d1 + d2 > 1) continue;
                        const int D = d1 + d2 - att(k1, h2, d) - att(h1, k2, d) + att(h1, h2, d) + att(k1, k2, d);
                        if (D < bD) bD = D, b1 = c1, b2 = c2, bk1 = k1, bk2 = k2;  // strictly: the first of the smallest in (c1, c2, k1, k2) order
                    }
                }
            }
        }
        if (bD >= 0) return false;
        h[(size_t)b1] = (uint8_t)bk1, h[(size_t)b2] = (uint8_t)bk2;
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
    if (q->N <= 4) launch_hop<4>(a, pairs, s);
    else if (q->N <= 8) launch_hop<8>(a, pairs, s);
    else if (q->N <= 12) launch_hop<12>(a, pairs, s);
    else if (q->N <= 16) launch_hop<16>(a, pairs, s);
    else if (q->N <= 24) launch_hop<24>(a, pairs, s);
    else launch_hop<32>(a, pairs, s);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(g_hop_err, MCQ_EDEVICE, "mcq_hop_device: %s", hipGetErrorString(e));
    return MCQ_OK;
}

}  // extern "C"
