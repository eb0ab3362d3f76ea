// mcq_table.h -- the BOARD TABLE, which csrc/mcq_quench_pairs.hip, csrc/mcq_hop.hip and csrc/mcq_tabu.hip live on: its device form in LDS, the
// single-move pass and the pair scan over it, their host forms, and the choice of an instantiation.  a(c, k) = the number of queens that
// attack height k of column c = (i, j), one entry per (c, k); a(c, h[c]) summed over the columns is 2 E.
//
//   layout  one chain per wavefront, one wavefront per workgroup (64 lanes), in the kernel's own __shared__ arrays:
//             h       the chain's N^2 heights, a byte each
//             tab32   the WHOLE table as one byte per entry (a <= 4 (N - 1) = 124) in rows of S bytes, S a multiple of 4 with an odd number of
//                     dwords, so that a lane per column reads its row as dwords without bank conflicts.  An entry behind k = N - 1 is 0xFF:
//                     it never wins an argmin and never has a difference of 0 or 1
//             mask0, mask1   for the scan alone, a word per column: the heights k != h with a(c, k) - a(c, h) = 0 and = 1
//   update  The table is built once (a gather, one lane per entry).  A move of column c then touches at most 6 entries in each of the
//           <= 4 (N - 1) aligned columns, one lane per aligned column (`apply`), so the table is exact behind every move.
//   barrier Every data-dependent loop is uniform over the wavefront (one chain), so __syncthreads() is legal wherever lanes hand LDS data to
//           each other; in a workgroup of one wavefront it is no hardware barrier, only the wait for the LDS counter and a fence for the
//           compiler.  The functions here hold the ones their own steps need.
//   host    the same rules over host buffers with plain loops and a table of ints that is recounted, never updated; the callers own the
//           buffers and pass pointers into them.
#ifndef MCQ_TABLE_H
#define MCQ_TABLE_H

#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "mcq_post.h"

namespace mcq_table {

__host__ __device__ __forceinline__ int att(int k, int kk, int d) {
    const int x = k > kk ? k - kk : kk - k;
    return (x == 0) | (x == d);
}

// the scan's key: D + 4 above c1, c2, k1, k2 (10 bits each), so that the smallest key is the lexicographically smallest candidate
constexpr unsigned long long PAIR_KEY_NONE = 4ull << 40;  // D = 0: no candidate improves
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

// ---- the instantiations ----
// the rows of a board padded to NP: columns, dwords and bytes of a table row, dwords of a row that hold entries
template <int NP_>
struct Rows {
    static constexpr int NP = NP_, QP = NP * NP;
    static constexpr int SW = (NP / 4) | 1, S = 4 * SW;
    static constexpr int RW = NP / 4;
};

template <class F>
auto for_rows_of(int N, F&& f) {
    if (N <= 4) return f(Rows<4>{});
    if (N <= 8) return f(Rows<8>{});
    if (N <= 12) return f(Rows<12>{});
    if (N <= 16) return f(Rows<16>{});
    if (N <= 24) return f(Rows<24>{});
    return f(Rows<32>{});
}

// ---- device: the start of a chain ----
// a byte of the chain's input as a height: clamped to N - 1
__host__ __device__ __forceinline__ uint8_t clamped(int v, int N) { return (uint8_t)(v < N ? v : N - 1); }

// 0xFF into every byte of the table: what lies behind k = N - 1 never wins an argmin.  No barrier: a caller with LDS of its own to prepare
// does that next, and then holds the one barrier in front of `build`
template <int NP>
__device__ __forceinline__ void fill(uint32_t* tab32, int Q, int lane) {
    for (int w = lane; w < Q * Rows<NP>::SW; w += 64) tab32[w] = 0xFFFFFFFFu;
}

// the table of the heights in h, one lane per entry, and the barrier behind it
template <int NP>
__device__ __forceinline__ void build(uint32_t* tab32, const uint8_t* h, int N, int lane) {
    uint8_t* tab = reinterpret_cast<uint8_t*>(tab32);
    const int Q = N * N;
    for (int e = lane; e < Q * N; e += 64) {
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
        tab[c * Rows<NP>::S + k] = (uint8_t)cnt;
    }
    __syncthreads();
}

// E of the heights in h from an exact table, in every lane
template <int NP>
__device__ __forceinline__ int energy(const uint32_t* tab32, const uint8_t* h, int N, int lane) {
    const uint8_t* tab = reinterpret_cast<const uint8_t*>(tab32);
    int twoE = 0;
    for (int c = lane; c < N * N; c += 64) twoE += tab[c * Rows<NP>::S + h[c]];
    for (int o = 32; o; o >>= 1) twoE += __shfl_xor(twoE, o);
    return twoE >> 1;
}

// the start of a chain for a kernel with nothing of its own in between: the clamped input into h, the table, E
template <int NP>
__device__ __forceinline__ int start(uint32_t* tab32, uint8_t* h, const uint8_t* in, int N, int lane) {
    const int Q = N * N;
    for (int c = lane; c < Q; c += 64) h[c] = clamped(in[c], N);
    fill<NP>(tab32, Q, lane);
    __syncthreads();
    build<NP>(tab32, h, N, lane);
    return energy<NP>(tab32, h, N, lane);
}

// ---- device: moves ----
// column c takes the height hn: the table rows of its aligned columns follow, one lane per aligned column
template <int NP>
__device__ __forceinline__ void apply(uint32_t* tab32, uint8_t* h, int N, int lane, int c, int hn) {
    uint8_t* tab = reinterpret_cast<uint8_t*>(tab32);
    const int i = c / N, j = c - i * N, ho = h[c];
    for (int t = lane; t < 4 * N; t += 64) {
        int c2, d;
        if (!aligned_slot(N, i, j, t, c2, d)) continue;
        uint8_t* row = tab + c2 * Rows<NP>::S;
        row[ho]--;
        if (ho - d >= 0) row[ho - d]--;
        if (ho + d < N) row[ho + d]--;
        row[hn]++;
        if (hn - d >= 0) row[hn - d]++;
        if (hn + d < N) row[hn + d]++;
    }
    h[c] = (uint8_t)hn;
    __syncthreads();
}

// one pass of the single-move rule: a lane per column, 64 columns at a time from a cursor.  Every lane takes the argmin of its table row,
// a ballot finds the first column that improves, that move is applied, and the cursor goes on behind it: the row-major pass of the rule,
// because the table is exact behind every move.  Returns the number of moves; E follows them.  (The loop of passes is the caller's.)
template <int NP>
__device__ __forceinline__ int pass(uint32_t* tab32, uint8_t* h, int N, int lane, int& E) {
    using R = Rows<NP>;
    const uint8_t* tab = reinterpret_cast<const uint8_t*>(tab32);
    const int Q = N * N;
    int moved = 0;
    for (int cur = 0; cur < Q;) {
        const int c = cur + lane;
        int key = INT_MAX, now = 0;
        if (c < Q) {
            const uint32_t* row = tab32 + c * R::SW;
#pragma unroll
            for (int w = 0; w < R::RW; w++) {
                const uint32_t v = row[w];
#pragma unroll
                for (int b = 0; b < 4; b++) key = min(key, (int)((((v >> (8 * b)) & 255u) << 8) | (uint32_t)(4 * w + b)));
            }
            now = tab[c * R::S + h[c]];
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
        apply<NP>(tab32, h, N, lane, cur + first, kbest);
        cur += first + 1;
    }
    return moved;
}

// the smallest key over the aligned pairs; PAIR_KEY_NONE or above when no pair improves.  Behind a descent every single-move difference
// is >= 0 and the four att terms add >= -2, so D < 0 needs delta1 + delta2 <= 1: columns where mask0 and mask1 are both empty -- nearly
// all of them on a real plateau -- take no part.  For every other column c1 the lanes take the aligned columns c2 > c1 and walk the set
// bits; one __shfl_xor butterfly reduces the running minimum.
template <int NP>
__device__ __forceinline__ unsigned long long scan(const uint32_t* tab32, const uint8_t* h, uint32_t* mask0, uint32_t* mask1, int N, int lane) {
    using R = Rows<NP>;
    const uint8_t* tab = reinterpret_cast<const uint8_t*>(tab32);
    const int Q = N * N;
    for (int c = lane; c < Q; c += 64) {
        const int hc = h[c], now = tab[c * R::S + hc];
        const uint32_t* row = tab32 + c * R::SW;
        uint32_t m0 = 0, m1 = 0;
#pragma unroll
        for (int w = 0; w < R::RW; w++) {
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
}

// ---- host ----
// h: N^2 heights; T: a table of N^3 ints, row c = a(c, .); a: one row of N ints; light: N^2 ints

// the chain's bytes, clamped to N - 1
inline void host_load(const uint8_t* in, int N, uint8_t* h) {
    for (int c = 0; c < N * N; c++) h[c] = clamped(in[c], N);
}

// the recount: every row of T from the heights, and E
inline int host_table(const uint8_t* h, int N, int* T) {
    long long twoE = 0;
    for (int c = 0; c < N * N; c++) {
        mcq_post::host_counts(h, N, c / N, c % N, T + (size_t)c * N);
        twoE += T[(size_t)c * N + h[c]];
    }
    return (int)(twoE / 2);
}

// one pass of the single-move rule over recounted rows.  Returns the number of moves; E follows them
inline int host_pass(uint8_t* h, int N, int* a, int& E) {
    int moved = 0;
    for (int c = 0; c < N * N; c++) {
        mcq_post::host_counts(h, N, c / N, c % N, a);
        int best = 0;
        for (int k = 1; k < N; k++)
            if (a[k] < a[best]) best = k;  // strictly: the smallest k of the minimum
        const int now = a[h[c]];
        if (a[best] < now) {
            h[c] = (uint8_t)best;
            E += a[best] - now;
            moved++;
        }
    }
    return moved;
}

// the best pair move of a single-move minimum: columns c1 < c2 take k1, k2 and E changes by D < 0; D = 0 when no pair improves
struct HostPair {
    int D, c1, c2, k1, k2;
};

// the scan over the rebuilt table T: the first of the smallest D in (c1, c2, k1, k2) order
inline HostPair host_scan(const uint8_t* h, int N, int* T, int* light) {
    const int Q = N * N;
    host_table(h, N, T);
    for (int c = 0; c < Q; c++) {
        const int* row = T + (size_t)c * N;
        light[c] = 0;  // a column without a height k != h of difference <= 1 is in no improving pair
        for (int k = 0; k < N; k++)
            if (k != h[c] && row[k] - row[h[c]] <= 1) light[c] = 1;
    }
    HostPair p{0, -1, -1, -1, -1};
    for (int c1 = 0; c1 < Q; c1++) {
        if (!light[c1]) continue;
        const int i1 = c1 / N, j1 = c1 % N, h1 = h[c1];
        const int* r1 = T + (size_t)c1 * N;
        for (int c2 = c1 + 1; c2 < Q; c2++) {
            if (!light[c2]) continue;
            const int di = c2 / N - i1, dj = c2 % N - j1, adi = di < 0 ? -di : di, adj = dj < 0 ? -dj : dj;
            if (!(di == 0 || dj == 0 || adi == adj)) continue;
            const int d = adi > adj ? adi : adj, h2 = h[c2];
            const int* r2 = T + (size_t)c2 * N;
            for (int k1 = 0; k1 < N; k1++) {
                const int d1 = r1[k1] - r1[h1];
                if (k1 == h1 || d1 > 1) continue;
                for (int k2 = 0; k2 < N; k2++) {
                    const int d2 = r2[k2] - r2[h2];
                    if (k2 == h2 || d1 + d2 > 1) continue;
                    const int D = d1 + d2 - att(k1, h2, d) - att(h1, k2, d) + att(h1, h2, d) + att(k1, k2, d);
                    if (D < p.D) p = HostPair{D, c1, c2, k1, k2};  // strictly: the first of the smallest
                }
            }
        }
    }
    return p;
}

}  // namespace mcq_table

#endif
