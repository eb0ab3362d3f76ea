// mcq_quench_pairs.hip -- the pair-move quench: board placements descend to a minimum under single-height moves and under moves of two
// aligned columns at once (include/mcq.h: mcq_quench_pairs, where the rule is stated).  It sits outside the sweep like
// csrc/mcq_quench.hip: placements in device memory in, placements and per-chain figures out, nothing goes to the host.
//
//   kernel  one chain per wavefront, one wavefront per workgroup, on the board table of csrc/mcq_table.h: the layout in LDS, the start of
//           a chain, `apply`, the pass of the single-move descent and the pair scan are there.  This file keeps the LDS arrays, the loop
//           of passes with its guard, the loop of rounds and the figures.  A changed height is stored by every lane, as
//           mcq_quench_kernel does.
//   host    mcq_quench_pairs_host: the same rule over host buffers with plain loops and a table rebuilt per round.
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

template <int NP>
__global__ __launch_bounds__(64) void mcq_quench_pairs_kernel(PairsArgs a) {
    using R = mcq_table::Rows<NP>;
    constexpr int QP = R::QP, SW = R::SW, S = R::S;
    __shared__ uint32_t tab32[QP * SW];
    __shared__ uint32_t mask0[QP], mask1[QP];
    __shared__ uint8_t h[QP];
    const uint8_t* tab = reinterpret_cast<const uint8_t*>(tab32);
    const int N = a.N, Q = N * N;
    const int lane = threadIdx.x;
    const long long ch = blockIdx.x;
    const int e_in = mcq_table::start<NP>(tab32, h, a.state_in + ch * Q, N, lane);
    int E = e_in, moves = 0, pair_moves = 0, rounds = 0, certified = 0;

    // column c takes the height hn, and the table follows
    auto apply = [&](int c, int hn) { mcq_table::apply<NP>(tab32, h, N, lane, c, hn); };

    // passes of the single-move rule until one moves nothing
    auto descend = [&]() {
        for (;;) {
            const int moved = mcq_table::pass<NP>(tab32, h, N, lane, E);
            moves += moved;
            // (moves + pair_moves > e_in cannot happen -- every move lowers E --: it only bounds the loop should the rule ever be broken)
            if (moved == 0 || moves + pair_moves > e_in) break;
        }
    };

    descend();
    const int e_single = E;
    for (;;) {
        rounds++;
        const unsigned long long key = mcq_table::scan<NP>(tab32, h, mask0, mask1, N, lane);
        if (key >= mcq_table::PAIR_KEY_NONE) {
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

// one chain in host code
void host_chain(const mcq_quench_pairs* q, long long ch) {
    const int N = q->N, Q = N * N;
    std::vector<uint8_t> h((size_t)Q);
    std::vector<int> a((size_t)N), T((size_t)Q * N), light((size_t)Q);
    mcq_table::host_load(q->state_in + ch * Q, N, h.data());
    const int e_in = mcq_table::host_table(h.data(), N, T.data());
    int E = e_in, moves = 0, pair_moves = 0, rounds = 0, certified = 0;
    auto descend = [&]() {
        for (;;) {
            const int moved = mcq_table::host_pass(h.data(), N, a.data(), E);
            moves += moved;
            if (moved == 0) break;
        }
    };
    descend();
    const int e_single = E;
    for (;;) {
        rounds++;
        const mcq_table::HostPair p = mcq_table::host_scan(h.data(), N, T.data(), light.data());
        if (p.D >= 0) {
            certified = 1;
            break;
        }
        h[(size_t)p.c1] = (uint8_t)p.k1, h[(size_t)p.c2] = (uint8_t)p.k2;
        E += p.D;
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
    mcq_table::for_rows_of(q->N, [&](auto rows) {
        hipLaunchKernelGGL((mcq_quench_pairs_kernel<decltype(rows)::NP>), dim3((unsigned)a.n_chains), dim3(64), 0, s, a);
    });
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(g_pairs_err, MCQ_EDEVICE, "mcq_quench_pairs_device: %s", hipGetErrorString(e));
    return MCQ_OK;
}

}  // extern "C"
