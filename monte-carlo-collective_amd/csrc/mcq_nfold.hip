// mcq_nfold.hip -- the n-fold way of Bortz, Kalos and Lebowitz for board placements: the Metropolis dynamics of the reference's move
// without its rejections (include/mcq.h: mcq_nfold, where the rule is stated).  Every accepted move of a board has a weight, the next
// event is drawn in proportion to it, and the clock advances by the time the Metropolis chain would have spent rejecting.  The table
// a(c, k), `start`, `apply` and `for_rows_of` are those of csrc/mcq_table.h; what this file adds is the weight R(c) of every column,
// the draw over them and the clock.
//
//   kernel  one chain per wavefront, one wavefront per workgroup, as in the hops.  LDS holds the WHOLE table a(c, k) in the layout of
//           csrc/mcq_table.h, the heights h and the best placement (N^2 bytes each), R(c) = sum over k != h(c) of w(c, k) as one dword
//           per column, the staged weight row T_s (table_len dwords) and the clock table (256 dwords).
//           R: lane l owns the CH = ceil(NP^2 / 64) consecutive columns l CH .. l CH + CH - 1, kept ST = CH | 1 dwords apart from the next
//           lane's, so that the lanes' reads of their chunks fall into different banks.  Columns behind N^2 hold 0 and are never written.
//           EVENT: every lane sums its chunk (uint64: 16 columns of up to 31 2^24), a 64-bit inclusive scan over the wavefront gives the
//           prefix sums and, in lane 63, W.  One 64-bit division gives tau.  When the event fires, U = the high half of X W, a ballot
//           finds the first lane whose prefix exceeds U, all lanes walk that lane's CH columns (the same LDS words in every lane), and a
//           lane per height k forms w(c, k), a 32-bit scan and a second ballot find k.  Then `apply`, and R is formed again for the moved
//           column and its <= 4 (N - 1) aligned columns only, a lane per column over the slots `apply` walks: no other column has a
//           changed table row or a changed a(c, h(c)).
//           SEGMENT: the row T_s is staged and every R is formed again, a lane per column.
//   host    mcq_nfold_host: the same rule over host buffers with plain loops; a table of ints whose rows are recounted behind every
//           event (mcq_post::host_counts), every R summed again, and a linear walk over (c, k).
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

thread_local char g_nfold_err[256] = "";

constexpr uint32_t NFOLD_KEY_WORD = 11u;  // key word 1 of the chain's Philox stream: 0 - 10 are taken (include/mcq.h: mcq_nfold, item 5)
constexpr int TB = MCQ_NFOLD_TIME_BITS;

struct NfoldArgs {
    const uint32_t* seeds;
    const uint32_t* table;
    const uint32_t* clock_table;
    const uint64_t* need_in;
    const int64_t* events_in;
    const uint8_t* state_in;
    uint8_t* state_out;
    uint8_t* best_state;
    int32_t* energy_in;
    int32_t* energy_out;
    int32_t* best_energy;
    int64_t* best_step;
    int64_t* events_out;
    int64_t* n_uphill;
    int64_t* n_flat;
    uint64_t* need_out;
    uint64_t* weight_out;
    int32_t* energy_hist;
    long long hist_stride;
    long long n_chains;
    long long n_segs;
    long long seg_steps;
    uint32_t clock_ln2;
    int table_len;
    int N;
};

// the per-chain figures, by one lane or by the host: `a` is the kernel's argument struct or the parameter block
template <class A>
__host__ __device__ __forceinline__ void store_nfold_figures(const A& a, long long ch, int e_in, int E, int best_e, long long best_step,
                                                             unsigned long long events, long long up, long long flat, unsigned long long need,
                                                             unsigned long long W) {
    if (a.energy_in) a.energy_in[ch] = e_in;
    if (a.energy_out) a.energy_out[ch] = E;
    if (a.best_energy) a.best_energy[ch] = best_e;
    if (a.best_step) a.best_step[ch] = best_step;
    if (a.events_out) a.events_out[ch] = (int64_t)events;
    if (a.n_uphill) a.n_uphill[ch] = up;
    if (a.n_flat) a.n_flat[ch] = flat;
    if (a.need_out) a.need_out[ch] = need;
    if (a.weight_out) a.weight_out[ch] = W;
}

// l(x) of rule item 5: z clock_ln2 + clock_table[y], z the leading zero bits of x and y the 8 bits below its leading one bit
__host__ __device__ __forceinline__ uint32_t clock_ell(uint32_t x, uint32_t ln2, const uint32_t* clock_table) {
    const int z = x ? __builtin_clz(x) : 32;
    const uint32_t y = x ? ((x << z) >> 23) & 255u : 0u;
    return (uint32_t)z * ln2 + clock_table[y];
}

// floor(a b / 2^64)
__host__ __device__ __forceinline__ unsigned long long mulhi64(unsigned long long a, unsigned long long b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    const unsigned long long a0 = a & 0xFFFFFFFFull, a1 = a >> 32, b0 = b & 0xFFFFFFFFull, b1 = b >> 32;
    const unsigned long long mid = a1 * b0 + ((a0 * b0) >> 32), mid2 = a0 * b1 + (mid & 0xFFFFFFFFull);
    return a1 * b1 + (mid >> 32) + (mid2 >> 32);
#endif
}

// w(c, k) of a difference d under the staged row: T[min(max(d, 0), D - 1)]
__host__ __device__ __forceinline__ uint32_t weight_of(const uint32_t* T, int d, int last) { return T[d < 0 ? 0 : d > last ? last : d]; }

// the dwords of R a lane keeps, and where column c lies among them
template <int NP>
struct Chunks {
    static constexpr int CH = (NP * NP + 63) / 64, ST = CH | 1;
    __device__ static __forceinline__ int at(int c) { return c + (c / CH) * (ST - CH); }
};

// R(c) from the table row of column c: the entries behind k = N - 1 and the column's own height carry no weight
template <int NP>
__device__ __forceinline__ uint32_t row_weight(const uint32_t* tab32, const uint8_t* h, const uint32_t* T, int last, int N, int c) {
    using R = mcq_table::Rows<NP>;
    const uint8_t* tab = reinterpret_cast<const uint8_t*>(tab32);
    const int hc = h[c], now = tab[c * R::S + hc];
    const uint32_t* row = tab32 + c * R::SW;
    uint32_t sum = 0;
#pragma unroll
    for (int w = 0; w < R::RW; w++) {
        const uint32_t v = row[w];
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const int k = 4 * w + b;
            const uint32_t wt = weight_of(T, (int)((v >> (8 * b)) & 255u) - now, last);
            sum += (k < N && k != hc) ? wt : 0u;
        }
    }
    return sum;
}

template <int NP>
constexpr int nfold_lds_bytes() {
    return NP * NP * (4 * ((NP / 4) | 1) + 2) + 4 * (64 * Chunks<NP>::ST + MCQ_MAX_NFOLD_TABLE + 256);
}

template <int NP>
__global__ __launch_bounds__(64) void mcq_nfold_kernel(NfoldArgs a) {
    using R = mcq_table::Rows<NP>;
    using K = Chunks<NP>;
    constexpr int QP = R::QP, SW = R::SW, S = R::S, CH = K::CH, ST = K::ST;
    __shared__ uint32_t tab32[QP * SW];
    __shared__ uint32_t Rs[64 * ST];
    __shared__ uint32_t T[MCQ_MAX_NFOLD_TABLE];
    __shared__ uint32_t clk[256];
    __shared__ uint8_t h[QP], best[QP];
    static_assert(sizeof(tab32) + sizeof(Rs) + sizeof(T) + sizeof(clk) + sizeof(h) + sizeof(best) == nfold_lds_bytes<NP>(), "the LDS of a chain");
    static_assert(nfold_lds_bytes<NP>() <= 64 * 1024, "a chain fits the LDS of a workgroup");
    const uint8_t* tab = reinterpret_cast<const uint8_t*>(tab32);
    const int N = a.N, Q = N * N, D = a.table_len, last = D - 1;
    const int lane = threadIdx.x;
    const long long ch = blockIdx.x;
    const uint32_t seed = a.seeds[ch];
    for (int i = lane; i < 64 * ST; i += 64) Rs[i] = 0;
    for (int i = lane; i < 256; i += 64) clk[i] = a.clock_table[i];
    int E = mcq_table::start<NP>(tab32, h, a.state_in + ch * Q, N, lane);
    for (int c = lane; c < Q; c += 64) best[c] = h[c];

    unsigned long long e = a.events_in ? (unsigned long long)a.events_in[ch] : 0ull;
    uint32_t x[4];
    mcq_post::philox_block((uint32_t)e, (uint32_t)(e >> 32), seed, NFOLD_KEY_WORD, x);
    const unsigned long long M = (unsigned long long)Q * (unsigned)(N - 1);
    unsigned long long need = a.need_in ? a.need_in[ch] : M * clock_ell(x[2], a.clock_ln2, clk);
    const int e_in = E;
    int best_e = E;
    long long best_step = 0, up = 0, flat = 0;
    unsigned long long W = 0;
    int32_t* hist = a.energy_hist ? a.energy_hist + ch * a.hist_stride : nullptr;
    if (hist && lane == 0) hist[0] = E;

    for (long long s = 0; s < a.n_segs; s++) {
        __syncthreads();  // (the row of the segment before has been read)
        for (int i = lane; i < D; i += 64) T[i] = a.table[s * D + i];
        __syncthreads();
        for (int c = lane; c < Q; c += 64) Rs[K::at(c)] = row_weight<NP>(tab32, h, T, last, N, c);
        __syncthreads();
        const unsigned long long whole = (unsigned long long)a.seg_steps << TB;
        unsigned long long left = whole;
        for (;;) {
            unsigned long long sum = 0;
#pragma unroll
            for (int i = 0; i < CH; i++) sum += Rs[lane * ST + i];
            unsigned long long incl = sum;
            for (int o = 1; o < 64; o <<= 1) {
                const unsigned long long t = __shfl_up(incl, o);
                incl += lane >= o ? t : 0ull;
            }
            W = __shfl(incl, 63);
            if (W == 0) break;  // a strict minimum under this row sleeps
            const unsigned long long q = (need << TB) / W, tau = q ? q : 1ull;
            if (tau > left) {
                need -= (left * W) >> TB;
                break;
            }
            left -= tau;

            // the move: the first (c, k) whose inclusive prefix sum exceeds U
            const unsigned long long U = mulhi64(((unsigned long long)x[0] << 32) | x[1], W);
            const int F = __ffsll(__ballot(incl > U)) - 1;  // (lane 63 holds W > U)
            unsigned long long u = U - __shfl(incl - sum, F);
            int ci = 0;
            bool found = false;
#pragma unroll
            for (int i = 0; i < CH; i++) {
                const uint32_t r = Rs[F * ST + i];
                if (!found) {
                    if (u < r) found = true, ci = i;
                    else u -= r;
                }
            }
            int c = F * CH + ci;
            c = c < Q ? c : Q - 1;  // (cannot happen -- a column behind N^2 holds 0 --: it only keeps a broken rule inside the arrays)
            const uint32_t u32 = (uint32_t)u;
            const int hc = h[c], now = tab[c * S + hc];
            int d = 0;
            uint32_t pk = 0;
            if (lane < N && lane != hc) {
                d = (int)tab[c * S + lane] - now;
                pk = weight_of(T, d, last);
            }
            for (int o = 1; o < 32; o <<= 1) {
                const uint32_t t = (uint32_t)__shfl_up((int)pk, o);
                pk += lane >= o ? t : 0u;
            }
            const unsigned long long hit = __ballot(lane < N && lane != hc && pk > u32);
            if (!hit) break;  // (cannot happen -- u < R(c) --: it only ends a broken rule)
            const int k = __ffsll(hit) - 1;
            const int dd = __shfl(d, k);
            mcq_table::apply<NP>(tab32, h, N, lane, c, k);
            E += dd, up += dd > 0, flat += dd == 0, e++;
            if (E < best_e) {
                best_e = E, best_step = s * a.seg_steps + (long long)((whole - left) >> TB);
                for (int cc = lane; cc < Q; cc += 64) best[cc] = h[cc];
            }
            // R of the moved column (slot t = j is its own place in its row) and of its aligned columns
            const int i0 = c / N, j0 = c - i0 * N;
            for (int t = lane; t < 4 * N; t += 64) {
                int c2, dist;
                bool ok = mcq_table::aligned_slot(N, i0, j0, t, c2, dist);
                if (t == j0) c2 = c, ok = true;
                if (ok) Rs[K::at(c2)] = row_weight<NP>(tab32, h, T, last, N, c2);
            }
            __syncthreads();
            mcq_post::philox_block((uint32_t)e, (uint32_t)(e >> 32), seed, NFOLD_KEY_WORD, x);
            need = M * clock_ell(x[2], a.clock_ln2, clk);
        }
        if (hist && lane == 0) hist[s + 1] = E;
    }

    uint8_t* out = a.state_out + ch * Q;
    for (int c = lane; c < Q; c += 64) out[c] = h[c];
    if (a.best_state) {
        uint8_t* bs = a.best_state + ch * Q;
        for (int c = lane; c < Q; c += 64) bs[c] = best[c];
    }
    if (lane == 0) store_nfold_figures(a, ch, e_in, E, best_e, best_step, e, up, flat, need, W);
}

constexpr long long STEP_LIMIT = 1ll << MCQ_NFOLD_STEP_BITS;

// what both entry points refuse
int check_nfold(const mcq_nfold* q) {
    if (!q) return fail(g_nfold_err, MCQ_EINVAL, "mcq_nfold: NULL parameter block");
    if (q->mode != MCQ_MODE_BOARD) return fail(g_nfold_err, MCQ_EINVAL, "mode: the n-fold way runs boards only (MCQ_MODE_BOARD), got %d", (int)q->mode);
    if (q->N < MCQ_MIN_N || q->N > MCQ_MAX_N_QUENCH_PAIRS)
        return fail(g_nfold_err, MCQ_EINVAL, "N out of range [%d, %d]: %d", MCQ_MIN_N, MCQ_MAX_N_QUENCH_PAIRS, (int)q->N);
    if (q->n_chains < 1 || q->n_chains > INT_MAX) return fail(g_nfold_err, MCQ_EINVAL, "n_chains out of range [1, 2^31 - 1]: %lld", (long long)q->n_chains);
    if (q->n_segs < 0) return fail(g_nfold_err, MCQ_EINVAL, "n_segs must be >= 0, got %lld", (long long)q->n_segs);
    if (q->first_seg < 0) return fail(g_nfold_err, MCQ_EINVAL, "first_seg must be >= 0, got %lld", (long long)q->first_seg);
    if (q->seg_steps < 1 || q->seg_steps > (1ll << 31)) return fail(g_nfold_err, MCQ_EINVAL, "seg_steps out of range [1, 2^31]: %lld", (long long)q->seg_steps);
    if (q->n_segs >= STEP_LIMIT || q->first_seg >= STEP_LIMIT || q->first_seg + q->n_segs > (STEP_LIMIT - 1) / q->seg_steps)
        return fail(g_nfold_err, MCQ_EINVAL, "(first_seg + n_segs) seg_steps must stay below 2^%d: (%lld + %lld) * %lld", MCQ_NFOLD_STEP_BITS,
                    (long long)q->first_seg, (long long)q->n_segs, (long long)q->seg_steps);
    if (q->table_len < 1 || q->table_len > MCQ_MAX_NFOLD_TABLE)
        return fail(g_nfold_err, MCQ_EINVAL, "table_len out of range [1, %d]: %lld", MCQ_MAX_NFOLD_TABLE, (long long)q->table_len);
    if (q->clock_ln2 < 0 || q->clock_ln2 > (1ll << MCQ_NFOLD_WEIGHT_BITS))
        return fail(g_nfold_err, MCQ_EINVAL, "clock_ln2 out of range [0, 2^%d]: %lld", MCQ_NFOLD_WEIGHT_BITS, (long long)q->clock_ln2);
    if (!q->seeds) return fail(g_nfold_err, MCQ_EINVAL, "seeds is required");
    if (!q->state_in) return fail(g_nfold_err, MCQ_EINVAL, "state_in is required");
    if (!q->state_out) return fail(g_nfold_err, MCQ_EINVAL, "state_out is required");
    if (!q->clock_table) return fail(g_nfold_err, MCQ_EINVAL, "clock_table is required");
    if (!q->table && q->n_segs > 0) return fail(g_nfold_err, MCQ_EINVAL, "table is required when n_segs > 0");
    if (q->best_state && (q->best_state == q->state_in || q->best_state == q->state_out))
        return fail(g_nfold_err, MCQ_EINVAL, "best_state must be distinct from state_in and state_out");
    if (q->energy_hist && q->hist_stride < q->n_segs + 1)
        return fail(g_nfold_err, MCQ_EINVAL, "hist_stride must be >= n_segs + 1 = %lld, got %lld", (long long)q->n_segs + 1, (long long)q->hist_stride);
    return MCQ_OK;
}

// what the host entry can also look at: the entries of the tables and of the carried values
int check_nfold_entries(const mcq_nfold* q) {
    const long long D = q->table_len;
    for (long long i = 0; i < q->n_segs * D; i++)
        if (q->table[i] > (1u << MCQ_NFOLD_WEIGHT_BITS))
            return fail(g_nfold_err, MCQ_EINVAL, "table[%lld][%lld] = %u exceeds 2^%d", i / D, i % D, q->table[i], MCQ_NFOLD_WEIGHT_BITS);
    for (int i = 0; i < 256; i++)
        if (q->clock_table[i] > (1u << MCQ_NFOLD_CLOCK_BITS))
            return fail(g_nfold_err, MCQ_EINVAL, "clock_table[%d] = %u exceeds 2^%d", i, q->clock_table[i], MCQ_NFOLD_CLOCK_BITS);
    for (long long ch = 0; ch < q->n_chains; ch++) {
        if (q->need_in && q->need_in[ch] >= (1ull << MCQ_NFOLD_NEED_BITS))
            return fail(g_nfold_err, MCQ_EINVAL, "need_in[%lld] = %llu is not below 2^%d", ch, (unsigned long long)q->need_in[ch], MCQ_NFOLD_NEED_BITS);
        if (q->events_in && q->events_in[ch] < 0) return fail(g_nfold_err, MCQ_EINVAL, "events_in[%lld] must be >= 0, got %lld", ch, (long long)q->events_in[ch]);
    }
    return MCQ_OK;
}

// one chain in host code: the rows of a table of ints are recounted behind every event, every R is summed again
void host_chain(const mcq_nfold* q, long long ch) {
    const int N = q->N, Q = N * N, last = (int)q->table_len - 1;
    std::vector<uint8_t> h((size_t)Q), best;
    std::vector<int> A((size_t)Q * N);
    std::vector<uint32_t> Rv((size_t)Q);
    mcq_table::host_load(q->state_in + ch * Q, N, h.data());
    best = h;
    const uint32_t seed = q->seeds[ch], ln2 = (uint32_t)q->clock_ln2;
    int E = mcq_table::host_table(h.data(), N, A.data());
    unsigned long long e = q->events_in ? (unsigned long long)q->events_in[ch] : 0ull;
    uint32_t x[4];
    mcq_post::philox_block((uint32_t)e, (uint32_t)(e >> 32), seed, NFOLD_KEY_WORD, x);
    const unsigned long long M = (unsigned long long)Q * (unsigned)(N - 1);
    unsigned long long need = q->need_in ? q->need_in[ch] : M * clock_ell(x[2], ln2, q->clock_table);
    const int e_in = E;
    int best_e = E;
    long long best_step = 0, up = 0, flat = 0;
    unsigned long long W = 0;
    int32_t* hist = q->energy_hist ? q->energy_hist + ch * q->hist_stride : nullptr;
    if (hist) hist[0] = E;
    for (long long s = 0; s < q->n_segs; s++) {
        const uint32_t* T = q->table + s * q->table_len;
        const unsigned long long whole = (unsigned long long)q->seg_steps << TB;
        unsigned long long left = whole;
        for (;;) {
            W = 0;
            for (int c = 0; c < Q; c++) {
                const int* row = A.data() + (size_t)c * N;
                uint32_t r = 0;
                for (int k = 0; k < N; k++)
                    if (k != h[(size_t)c]) r += weight_of(T, row[k] - row[h[(size_t)c]], last);
                Rv[(size_t)c] = r;
                W += r;
            }
            if (W == 0) break;
            const unsigned long long qt = (need << TB) / W, tau = qt ? qt : 1ull;
            if (tau > left) {
                need -= (left * W) >> TB;
                break;
            }
            left -= tau;
            const unsigned long long U = mulhi64(((unsigned long long)x[0] << 32) | x[1], W);
            unsigned long long prefix = 0;
            int c = 0;
            while (prefix + Rv[(size_t)c] <= U) prefix += Rv[(size_t)c++];  // (U < W: the walk ends inside the board)
            const int* row = A.data() + (size_t)c * N;
            const int hc = h[(size_t)c];
            int k = 0, dd = 0;
            for (;; k++) {
                if (k == hc) continue;
                dd = row[k] - row[hc];
                prefix += weight_of(T, dd, last);
                if (prefix > U) break;
            }
            h[(size_t)c] = (uint8_t)k;
            const int i = c / N, j = c % N;
            for (int c2 = 0; c2 < Q; c2++) {  // the rows of the aligned columns are recounted
                const int di = c2 / N - i, dj = c2 % N - j, adi = di < 0 ? -di : di, adj = dj < 0 ? -dj : dj;
                if (c2 == c || !(di == 0 || dj == 0 || adi == adj)) continue;
                mcq_post::host_counts(h.data(), N, c2 / N, c2 % N, A.data() + (size_t)c2 * N);
            }
            E += dd, up += dd > 0, flat += dd == 0, e++;
            if (E < best_e) best_e = E, best_step = s * q->seg_steps + (long long)((whole - left) >> TB), best = h;
            mcq_post::philox_block((uint32_t)e, (uint32_t)(e >> 32), seed, NFOLD_KEY_WORD, x);
            need = M * clock_ell(x[2], ln2, q->clock_table);
        }
        if (hist) hist[s + 1] = E;
    }
    uint8_t* out = q->state_out + ch * Q;
    for (int c = 0; c < Q; c++) out[c] = h[(size_t)c];
    if (q->best_state)
        for (int c = 0; c < Q; c++) q->best_state[ch * Q + c] = best[(size_t)c];
    store_nfold_figures(*q, ch, e_in, E, best_e, best_step, e, up, flat, need, W);
}

}  // namespace

extern "C" {

const char* mcq_nfold_last_error(void) { return g_nfold_err; }

int mcq_nfold_host(const mcq_nfold* q) {
    int rc = check_nfold(q);
    if (rc == MCQ_OK) rc = check_nfold_entries(q);
    if (rc != MCQ_OK) return rc;
    mcq_post::for_chains((long long)q->n_chains, [q](long long first, long long last) {
        for (long long ch = first; ch < last; ch++) host_chain(q, ch);
    });
    return MCQ_OK;
}

int mcq_nfold_device(const mcq_nfold* q, void* hip_stream) {
    const int rc = check_nfold(q);
    if (rc != MCQ_OK) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    const NfoldArgs a{q->seeds, q->table, q->clock_table, q->need_in, q->events_in, q->state_in, q->state_out, q->best_state, q->energy_in, q->energy_out,
                      q->best_energy, q->best_step, q->events_out, q->n_uphill, q->n_flat, q->need_out, q->weight_out, q->energy_hist,
                      (long long)q->hist_stride, (long long)q->n_chains, (long long)q->n_segs, (long long)q->seg_steps, (uint32_t)q->clock_ln2,
                      (int)q->table_len, (int)q->N};
    mcq_table::for_rows_of(q->N, [&](auto rows) {
        constexpr int NP = decltype(rows)::NP;
        hipLaunchKernelGGL((mcq_nfold_kernel<NP>), dim3((unsigned)a.n_chains), dim3(64), 0, s, a);
    });
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(g_nfold_err, MCQ_EDEVICE, "mcq_nfold_device: %s", hipGetErrorString(e));
    return MCQ_OK;
}

}  // extern "C"
