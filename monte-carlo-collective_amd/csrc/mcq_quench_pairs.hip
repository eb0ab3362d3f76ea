// mcq_quench_pairs.hip -- the pair-move quench: board placements descend to a minimum under single-height moves and under moves of two
// aligned columns at once (include/mcq.h: mcq_quench_pairs, where the rule is stated).  It sits outside the sweep like
// csrc/mcq_quench.hip: placements in device memory in, placements and per-chain figures out, nothing goes to the host.
//
//   kernel  one chain per wavefront, one wavefront per workgroup.  LDS holds the chain's N^2 heights, the WHOLE table a(c, k) as one
//           byte per entry (a <= 4 (N - 1) = 124) in rows of S bytes, S a multiple of 4 with an odd number of dwords, so that a lane
//           per column reads its row as dwords without bank conflicts, and two words per column for the scan (below).  The table is
//           built once (a gather, one lane per entry); a move of column c then touches at most 6 entries in each of the <= 4 (N - 1)
//           aligned columns, one lane per aligned column.
//           DESCENT: a lane per column, 64 columns at a time from a cursor: every lane takes the argmin of its table row, a ballot
//           finds the first column that improves, that move is applied, and the cursor goes on behind it.  This is the row-major
//           pass of the rule, because the table is exact behind every move.
//           SCAN: behind a descent every single-move difference is >= 0 and the four att terms add >= -2, so D < 0 needs
//           delta1 + delta2 <= 1.  Per column two words hold the heights k != h with delta = 0 and with delta = 1; columns where both
//           are empty -- nearly all of them on a real plateau -- take no part.  For every other column c1 the lanes take the aligned
//           columns c2 > c1 and walk the set bits.  The running minimum is a packed 64-bit key, D + 4 above c1, c2, k1, k2; one
//           __shfl_xor butterfly per scan reduces it.
//           Every data-dependent loop is uniform over the wavefront (one chain), so __syncthreads() is legal wherever lanes hand
//           LDS data to each other; in a workgroup of one wavefront it is no hardware barrier, only the wait for the LDS counter and
//           a fence for the compiler.  A changed height is stored by every lane, as mcq_quench_kernel does.
//   host    mcq_quench_pairs_host: the same rule over host buffers with plain loops and a table rebuilt per round.
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

thread_local char g_pairs_err[256] = "";

struct PairsArgs {
    const uint8_t* state_in;
    uint8_t* state_out;
    int32_t* energy_in;
    int32_t* energy_single;
    int32_t* energy_out;
    int32_t* n_moves;
    int32_t* n_pair_moves;
    int32_t* n_rounds;
    int32_t* certified;
    uint16_t* conflicts;
    long long n_chains;
    long long max_rounds;
    int N;
};

// the per-chain figures, by one lane or by the host: `a` is the kernel's argument struct or the parameter block
template <class A>
__host__ __device__ __forceinline__ void store_pairs_figures(const A& a, long long ch, int e_in, int e_single, int E, int moves, int pair_moves,
                                                             int rounds, int certified) {
    if (a.energy_in) a.energy_in[ch] = e_in;
    if (a.energy_single) a.energy_single[ch] = e_single;
    if (a.energy_out) a.energy_out[ch] = E;
    if (a.n_moves) a.n_moves[ch] = moves;
    if (a.n_pair_moves) a.n_pair_moves[ch] = pair_moves;
    if (a.n_rounds) a.n_rounds[ch] = rounds;
    if (a.certified) a.certified[ch] = certified;
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

template <int NP>
__global__ __launch_bounds__(64) void mcq_quench_pairs_kernel(PairsArgs a) {
    constexpr int QP = NP * NP;
    constexpr int SW = (NP / 4) | 1, S = 4 * SW;  // dwords and bytes of a table row
    constexpr int RW = NP / 4;                    // dwords of a row that hold entries
    __shared__ uint32_t tab32[QP * SW];
    __shared__ uint32_t mask0[QP], mask1[QP];
    __shared__ uint8_t h[QP];
    uint8_t* tab = reinterpret_cast<uint8_t*>(tab32);
    const int N = a.N, Q = N * N;
    const int lane = threadIdx.x;
    const long long ch = blockIdx.x;
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
    int E = e_in, moves = 0, pair_moves = 0, rounds = 0, certified = 0;

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
            moves += moved;
            // (moves + pair_moves > e_in cannot happen -- every move lowers E --: it only bounds the loop should the rule ever be broken)
            if (moved == 0 || moves + pair_moves > e_in) break;
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

    descend();
    const int e_single = E;
    for (;;) {
        rounds++;
        const unsigned long long key = scan();
        if (key >= KEY_NONE) {
            certified = 1;
            break;
        }
        const int D = (int)(key >> 40) - 4;
        apply((int)(key >> 30) & 1023, (int)(key >> 10) & 1023);
        apply((int)(key >> 20) & 1023, (int)key & 1023);
        E += D;
        pair_moves++;
        descend();
        if ((a.max_rounds > 0 && rounds >= a.max_rounds) || moves + pair_moves > e_in) break;
    }

    uint8_t* out = a.state_out + ch * Q;
    for (int c = lane; c < Q; c += 64) out[c] = h[c];
    if (a.conflicts) {
        uint16_t* cf = a.conflicts + ch * Q;
        for (int c = lane; c < Q; c += 64) cf[c] = (uint16_t)tab[c * S + h[c]];
    }
    if (lane == 0) store_pairs_figures(a, ch, e_in, e_single, E, moves, pair_moves, rounds, certified);
}

// what both entry points refuse
int check_pairs(const mcq_quench_pairs* q) {
    if (!q) return fail(g_pairs_err, MCQ_EINVAL, "mcq_quench_pairs: NULL parameter block");
    if (q->mode != MCQ_MODE_BOARD) return fail(g_pairs_err, MCQ_EINVAL, "mode: the pair-move quench runs boards only (MCQ_MODE_BOARD), got %d", (int)q->mode);
    if (q->N < MCQ_MIN_N || q->N > MCQ_MAX_N_QUENCH_PAIRS)
        return fail(g_pairs_err, MCQ_EINVAL, "N out of range [%d, %d]: %d", MCQ_MIN_N, MCQ_MAX_N_QUENCH_PAIRS, (int)q->N);
    if (q->n_chains < 1 || q->n_chains > INT_MAX) return fail(g_pairs_err, MCQ_EINVAL, "n_chains out of range [1, 2^31 - 1]: %lld", (long long)q->n_chains);
    if (q->max_rounds < 0) return fail(g_pairs_err, MCQ_EINVAL, "max_rounds must be >= 0 (0 = no limit), got %lld", (long long)q->max_rounds);
    if (!q->state_in) return fail(g_pairs_err, MCQ_EINVAL, "state_in is required");
    if (!q->state_out) return fail(g_pairs_err, MCQ_EINVAL, "state_out is required");
    return MCQ_OK;
}

template <int NP>
void launch_pairs(const PairsArgs& a, hipStream_t s) {
    hipLaunchKernelGGL((mcq_quench_pairs_kernel<NP>), dim3((unsigned)a.n_chains), dim3(64), 0, s, a);
}

// one chain in host code
void host_chain(const mcq_quench_pairs* q, long long ch) {
    const int N = q->N, Q = N * N;
    std::vector<uint8_t> h((size_t)Q);
    std::vector<int> a((size_t)N), T((size_t)Q * N), light((size_t)Q);
    const uint8_t* in = q->state_in + ch * Q;
    for (int c = 0; c < Q; c++) h[(size_t)c] = (uint8_t)(in[c] < N ? in[c] : N - 1);
    long long twoE = 0;
    for (int c = 0; c < Q; c++) {
        host_counts(h.data(), N, c / N, c % N, a.data());
        twoE += a[h[(size_t)c]];
    }
    const int e_in = (int)(twoE / 2);
    int E = e_in, moves = 0, pair_moves = 0, rounds = 0, certified = 0;
    auto descend = [&]() {
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
            moves += moved;
            if (moved == 0) break;
        }
    };
    descend();
    const int e_single = E;
    for (;;) {
        rounds++;
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
        if (bD >= 0) {
            certified = 1;
            break;
        }
        h[(size_t)b1] = (uint8_t)bk1, h[(size_t)b2] = (uint8_t)bk2;
        E += bD;
        pair_moves++;
        descend();
        if (q->max_rounds > 0 && rounds >= q->max_rounds) break;
    }
    if (q->conflicts)
        for (int c = 0; c < Q; c++) {
            host_counts(h.data(), N, c / N, c % N, a.data());
            q->conflicts[ch * Q + c] = (uint16_t)a[h[(size_t)c]];
        }
    uint8_t* out = q->state_out + ch * Q;
    for (int c = 0; c < Q; c++) out[c] = h[(size_t)c];
    store_pairs_figures(*q, ch, e_in, e_single, E, moves, pair_moves, rounds, certified);
}

}  // namespace

extern "C" {

const char* mcq_quench_pairs_last_error(void) { return g_pairs_err; }

int mcq_quench_pairs_host(const mcq_quench_pairs* q) {
    const int rc = check_pairs(q);
    if (rc != MCQ_OK) return rc;
    mcq_post::for_chains((long long)q->n_chains, [q](long long first, long long last) {
        for (long long ch = first; ch < last; ch++) host_chain(q, ch);
    });
    return MCQ_OK;
}

int mcq_quench_pairs_device(const mcq_quench_pairs* q, void* hip_stream) {
    const int rc = check_pairs(q);
    if (rc != MCQ_OK) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    const PairsArgs a{q->state_in, q->state_out, q->energy_in, q->energy_single, q->energy_out, q->n_moves, q->n_pair_moves, q->n_rounds,
                      q->certified, q->conflicts, (long long)q->n_chains, (long long)q->max_rounds, (int)q->N};
    if (q->N <= 4) launch_pairs<4>(a, s);
    else if (q->N <= 8) launch_pairs<8>(a, s);
    else if (q->N <= 12) launch_pairs<12>(a, s);
    else if (q->N <= 16) launch_pairs<16>(a, s);
    else if (q->N <= 24) launch_pairs<24>(a, s);
    else launch_pairs<32>(a, s);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(g_pairs_err, MCQ_EDEVICE, "mcq_quench_pairs_device: %s", hipGetErrorString(e));
    return MCQ_OK;
}

}  // extern "C"
