// mcq_post.h -- what the kernels that sit outside the sweep share beyond the attack field (csrc/mcq_field.h): csrc/mcq_quench.hip,
// mcq_heatbath.hip, mcq_quench3d.hip and mcq_heatbath3d.hip.  Philox for the two heat baths, the host count a(c, k) of the board files,
// the stamp base of the two tabu searches, the error text behind every mcq_*_last_error, and for the two full_3d files the threads of the
// host entry points and the refusals.
#ifndef MCQ_POST_H
#define MCQ_POST_H

#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <thread>
#include <vector>

#include "../../include/mcq.h"

namespace mcq_post {

// `code`, with the message in the feature's buffer (thread-local, one per feature: the ABI has one mcq_*_last_error each)
__attribute__((format(printf, 3, 4))) inline int fail(char (&err)[256], int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(err, sizeof err, fmt, ap);
    va_end(ap);
    return code;
}

// philox4x32-10: counter (c0, c1, 0, 0), key (k0, k1)
__host__ __device__ __forceinline__ void philox_block(uint32_t c0, uint32_t c1, uint32_t k0, uint32_t k1, uint32_t out[4]) {
    uint32_t c2 = 0, c3 = 0;
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1, c3 = (uint32_t)p0, c0 = n0, c2 = n2;
        k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
    }
    out[0] = c0, out[1] = c1, out[2] = c2, out[3] = c3;
}

// the stamp base of the two tabu searches (csrc/mcq_tabu.hip, csrc/mcq_tabu3d.hip): uint16 stamps are kept relative to a base that moves
// by REBASE every REBASE iterations.  rebase2: both uint16 halves of v less REBASE = 2^15, stopping at 0: a half with its top bit set
// loses that bit, any other half becomes 0
constexpr int REBASE = 1 << 15;  // (rebase2 is written for 2^15)
__device__ __forceinline__ uint32_t rebase2(uint32_t v) {
    const uint32_t keep = ((v & 0x80008000u) >> 15) * 0xFFFFu;
    return v & 0x7FFF7FFFu & keep;
}

// the per-chain figures of a heat-bath call, by one lane or by the host: `a` is a kernel's argument struct or a parameter block
template <class A>
__host__ __device__ __forceinline__ void store_heatbath_figures(const A& a, long long ch, int e_in, int E, int best, long long best_sweep, long long changed) {
    if (a.energy_in) a.energy_in[ch] = e_in;
    if (a.energy_out) a.energy_out[ch] = E;
    if (a.best_energy) a.best_energy[ch] = best;
    if (a.best_sweep) a.best_sweep[ch] = best_sweep;
    if (a.n_changed) a.n_changed[ch] = changed;
}

// ... and of a quench
template <class A>
__host__ __device__ __forceinline__ void store_quench_figures(const A& a, long long ch, int e_in, int E, int moves, int passes) {
    if (a.energy_in) a.energy_in[ch] = e_in;
    if (a.energy_out) a.energy_out[ch] = E;
    if (a.n_moves) a.n_moves[ch] = moves;
    if (a.n_passes) a.n_passes[ch] = passes;
}

// boards: a[k] = a(c, k) of column (i, j), k = 0 .. N - 1, from the heights h (the quench's rule, items 1 - 2)
inline void host_counts(const uint8_t* h, int N, int i, int j, int* a) {
    for (int k = 0; k < N; k++) a[k] = 0;
    auto hit = [&](int hp, int d) {
        a[hp]++;
        if (hp - d >= 0) a[hp - d]++;
        if (hp + d < N) a[hp + d]++;
    };
    for (int jj = 0; jj < N; jj++) {  // the row, and the two diagonal cells of board column jj
        if (jj == j) continue;
        const int d = jj > j ? jj - j : j - jj;
        hit(h[i * N + jj], d);
        if (i + d < N) hit(h[(i + d) * N + jj], d);
        if (i - d >= 0) hit(h[(i - d) * N + jj], d);
    }
    for (int ii = 0; ii < N; ii++)  // the board column
        if (ii != i) hit(h[ii * N + j], ii > i ? ii - i : i - ii);
}

// fn(first, last) over the chains 0 .. n - 1.  Chains do not interact: a few threads share them (a test compares 65 536 chains with a kernel)
template <class F>
void for_chains(long long n, F fn) {
    const unsigned hw = std::thread::hardware_concurrency();
    const long long n_threads = std::min<long long>(std::min<long long>(hw ? hw : 1, 16), (n + 63) / 64);
    if (n_threads <= 1) {
        fn(0LL, n);
    } else {
        std::vector<std::thread> pool;
        for (long long t = 0; t < n_threads; t++) pool.emplace_back(fn, n * t / n_threads, n * (t + 1) / n_threads);
        for (auto& t : pool) t.join();
    }
}

// the Q of a full_3d parameter block
template <class P>
int queens_of(const P* q) { return q->n_queens == 0 ? q->N * q->N : q->n_queens; }

// what the full_3d entry points refuse of N, n_queens and n_chains; `feature` completes the one message that names it
inline int check_full3d(char (&err)[256], const char* feature, int N, int n_queens, long long n_chains) {
    if (N > MCQ_MAX_N_QUENCH3D && N <= MCQ_MAX_N)
        return fail(err, MCQ_EINVAL, "N out of range [%d, %d]: %d (the full_3d %s stops at N = %d, where a cell index fits 15 bits; the sweep runs to %d)",
                    MCQ_MIN_N, MCQ_MAX_N_QUENCH3D, N, feature, MCQ_MAX_N_QUENCH3D, MCQ_MAX_N);
    if (N < MCQ_MIN_N || N > MCQ_MAX_N_QUENCH3D) return fail(err, MCQ_EINVAL, "N out of range [%d, %d]: %d", MCQ_MIN_N, MCQ_MAX_N_QUENCH3D, N);
    const int cells = N * N * N;
    if (n_queens != 0 && (n_queens < 2 || n_queens > cells - 1))
        return fail(err, MCQ_EINVAL, "n_queens out of range [2, N^3 - 1 = %d] (0 = N^2): %d", cells - 1, n_queens);
    if (n_chains < 1 || n_chains > INT_MAX) return fail(err, MCQ_EINVAL, "n_chains out of range [1, 2^31 - 1]: %lld", n_chains);
    return MCQ_OK;
}

}  // namespace mcq_post

#endif
