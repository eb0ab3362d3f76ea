// mcq_temper3d.hip -- parallel tempering of full_3d heat-bath queen sweeps, one ladder per workgroup (include/mcq.h: mcq_temper3d, where
// the rule is stated).  The sweep is that of csrc/mcq_heatbath3d.hip on the attack field of csrc/mcq_field.h, the exchange that of
// csrc/mcq_temper.hip; what is new is that the R attack fields of a ladder sit in ONE workgroup, each at the table row of its rung, and
// trade rungs between sweeps through LDS, so that a whole tempered full_3d run is one launch.
//
//   kernel  a WORKGROUP is one ladder, a CHAIN is W lanes of it: W = min(the W of mcq_field::for_shape_of(N), 1024 / R), so R W <= 1024;
//           BITS and STEPS are those of for_shape_of(N).  The instantiations (W, BITS, STEPS):
//             N <= 12       (64, 8, 32)                                       every R
//             N = 13 .. 19  (256, 8, 64) R = 2, 4   (128, 8, 64) R = 8        (64, 8, 64) R = 16 (N = 19: a table shorter than 512)
//             N = 20 .. 32  (512, 16, 64) R = 2     (256, 16, 64) R = 4       (128, 16, 64) R = 8
//           A chain starts at a multiple of 64 lanes, so a wavefront belongs to one chain.  Dynamic LDS per ladder:
//             R chain regions   red (32 dwords), scan (16 x uint64), win (2 dwords + pad): 72 dwords of the chain's OWN, then field, occ
//                               and queens through mcq_field::carve; a region is rounded up to 4 dwords
//             tab               R D dwords: the sweep's rows by rung, staged once per sweep by the whole ladder
//             3 R words         the event: energy by rung, slot by rung, rung by slot
//           bytes = 4 (R roundup4(72 + fw + bw + ceil(Q / 2)) + R D + 3 R) <= MCQ_MAX_TEMPER_LDS - MCQ_TEMPER3D_STATIC_LDS (the workgroup OR
//           of __syncthreads_or keeps 256 bytes of static LDS, a multiple of 16, in front); what fits is tabulated in include/mcq.h.
//           The queen update is mcq_heatbath3d_kernel's with chain-local indices: lane = threadIdx.x mod W, put(.., lane, W, SLOTS), the
//           run of field dwords from the lane, and the cross-wavefront halves of minimum, sum and scan through the chain's own red and
//           scan by the wavefront's index within the chain (block_min, block_sum, block_scan below).
//           An EVENT is mcq_temper_kernel's: lane 0 of each chain posts its energy and its slot under its rung; barrier; lane t of the
//           ladder decides pair t (X from global memory), writes the two new rungs and counts the accept in a register; barrier; every
//           chain reads its rung back.
//   barrier Every __syncthreads() is met by all R W lanes, also where a chain is one wavefront (W = 64), because every branch around
//           one is uniform over the workgroup:
//             - block_min / block_sum / block_scan branch on W alone, a template parameter;
//             - the loops over sweeps and queens run n_sweeps and Q times, the launch's numbers, the same for every chain;
//             - "some slot repeats" comes from __syncthreads_or over the workgroup, so all chains take the held path or none does;
//             - "is this sweep followed by an event" depends on first_sweep, s and K alone;
//             - what depends on a chain's own data (the one lane that walks its run again, W = 0, a new best) holds no barrier.
//   held    a REPEATED placement cannot enter a byte field, and a ladder with one cannot keep its barriers uniform if that slot
//           alone stood still: the whole ladder is handed back unmoved (rule item 4), with the pairwise recount as every energy.
//   host    mcq_temper3d_host: the same rule ladder by ladder with one HostField per slot.
//
// Built for gfx950 only, with csrc/mcq_hip.hip:  hipcc --offload-arch=gfx950 -O3 -ffp-contract=off
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <vector>

#include "../../include/mcq.h"
#include "mcq_field.h"
#include "mcq_post.h"

namespace {

using mcq_field::attackers_at;
using mcq_field::attacks;
using mcq_field::carve;
using mcq_field::cell_of;
using mcq_field::field_at;
using mcq_field::HostField;
using mcq_field::load_queen;
using mcq_field::occupy;
using mcq_field::packed_of;
using mcq_field::put;
using mcq_field::put_slot;
using mcq_field::set_pad_bits;
using mcq_field::store_queens;
using mcq_field::vacate;
using mcq_post::fail;
using mcq_post::philox_block;
using mcq_post::queens_of;

thread_local char g_temper3d_err[256] = "";

struct Temper3dArgs {
    const uint32_t* seeds;
    const uint32_t* table;
    const uint32_t* swap_table;
    const uint8_t* rung_in;
    uint8_t* rung_out;
    const uint8_t* state_in;
    uint8_t* state_out;
    int32_t* energy_in;
    int32_t* energy_out;
    int32_t* best_energy;
    int64_t* best_sweep;
    uint8_t* best_state;
    int64_t* n_changed;
    int32_t* energy_hist;
    int64_t* n_exchanges;
    uint8_t* rung_hist;
    int64_t* pair_accepted;
    int32_t* flags;
    long long hist_stride;
    long long n_sweeps;
    long long first_sweep;
    long long every;          // K
    long long events_before;  // floor(first_sweep / K)
    int table_len;
    int swap_len;
    int R;
    int chain_words;          // dwords of LDS per chain region
    int N;
    int Q;
};

constexpr int HDR = 72;  // dwords of a chain's red, scan and win

// word w of the exchange stream of a ladder whose slot 0 is seeded `seed`: key word 4
__host__ __device__ __forceinline__ uint32_t exchange_word(uint32_t seed, unsigned long long w) {
    uint32_t r[4];
    philox_block((uint32_t)(w >> 2), (uint32_t)(w >> 34), seed, 4u, r);
    const int e = (int)(w & 3);
    return e == 0 ? r[0] : e == 1 ? r[1] : e == 2 ? r[2] : r[3];
}

// rule item 3 for one pair: Delta = E_b - E_a, X = the pair's row of the event
__host__ __device__ __forceinline__ bool pair_swaps(int delta, const uint32_t* X, int DX, uint32_t seed0, unsigned long long w) {
    if (delta >= 0) return true;
    const long long d = -(long long)delta;
    return exchange_word(seed0, w) < X[d < DX - 1 ? d : DX - 1];
}

// ---- the cross-wavefront halves, per CHAIN: `wave` = the wavefront's index within its chain, red and scan the chain's own.  The
// barriers are the workgroup's: every chain of the ladder makes the same calls (file header).
template <int W>
__device__ __forceinline__ uint32_t block_min(uint32_t v, uint32_t* red, int wave) {
    for (int o = 32; o; o >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, o, 64));
    if (W == 64) return v;
    if ((threadIdx.x & 63) == 0) red[wave] = v;
    __syncthreads();
    v = red[0];
    for (int w = 1; w < W / 64; w++) v = min(v, red[w]);
    return v;
}

template <int W>
__device__ __forceinline__ int block_sum(int v, uint32_t* red, int wave) {
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o, 64);
    if (W == 64) return v;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[wave] = (uint32_t)v;
    __syncthreads();
    v = (int)red[0];
    for (int w = 1; w < W / 64; w++) v += (int)red[w];
    return v;
}

// DPP within a row of 16 lanes: the value of the lane `n` below, 0 where the row ends
template <int n>
__device__ __forceinline__ unsigned long long row_shr64(unsigned long long v) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)v, 0x110 + n, 0xF, 0xF, false);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(v >> 32), 0x110 + n, 0xF, 0xF, false);
    return (unsigned long long)hi << 32 | lo;
}

template <int lane>
__device__ __forceinline__ unsigned long long read_lane64(unsigned long long v) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, lane), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), lane);
    return (unsigned long long)hi << 32 | lo;
}

// EXCLUSIVE prefix sum of `own` over the lanes of the CHAIN in lane order; `total` = the chain's sum
template <int W>
__device__ __forceinline__ unsigned long long block_scan(uint32_t own, unsigned long long* scan, int wave, unsigned long long& total) {
    unsigned long long v = own;
    v += row_shr64<1>(v);
    v += row_shr64<2>(v);
    v += row_shr64<4>(v);
    v += row_shr64<8>(v);
    const unsigned long long r0 = read_lane64<15>(v), r1 = read_lane64<31>(v), r2 = read_lane64<47>(v), r3 = read_lane64<63>(v);
    const int lane = threadIdx.x & 63;
    v += (lane >= 16 ? r0 : 0ull) + (lane >= 32 ? r1 : 0ull) + (lane >= 48 ? r2 : 0ull);
    total = r0 + r1 + r2 + r3;
    v -= own;
    if (W == 64) return v;
    if (lane == 0) scan[wave] = total;
    __syncthreads();
    unsigned long long before = 0, all = 0;
    for (int w = 0; w < W / 64; w++) {
        const unsigned long long t = scan[w];
        before += w < wave ? t : 0ull;
        all += t;
    }
    total = all;
    return v + before;
}

template <int W, int BITS, int STEPS>
__global__ __launch_bounds__(1024) void mcq_temper3d_kernel(Temper3dArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    constexpr int CPD = 32 / BITS, SLOTS = 13 * STEPS;
    constexpr uint32_t MASK = (1u << BITS) - 1u;
    const int N = a.N, Q = a.Q, N2 = N * N, C = N2 * N, D = a.table_len, R = a.R;
    const int tl = threadIdx.x;                                         // lane of the ladder
    const int slot = __builtin_amdgcn_readfirstlane(tl / W);            // chain of the ladder (a wavefront belongs to one chain)
    const int lane = tl & (W - 1);                                      // lane of the chain
    const int wave = __builtin_amdgcn_readfirstlane(lane >> 6);         // the wavefront's index within its chain
    const int LT = R * W;
    const long long lad = blockIdx.x, ch = lad * R + slot;
    uint32_t* base = lds + slot * a.chain_words;
    uint32_t* red = base;
    unsigned long long* scan = (unsigned long long*)(base + 32);
    uint32_t* win = base + 64;
    const auto [field, occ, queens, fw, bw] = carve<BITS>(base + HDR, C);
    uint32_t* tab = lds + R * a.chain_words;                            // [R][D]: the sweep's rows by rung
    int* e_by_rung = (int*)(tab + R * D);
    int* slot_by_rung = e_by_rung + R;
    int* rung_by_slot = slot_by_rung + R;
    const uint8_t* in = a.state_in + ch * 3 * Q;
    uint8_t* out = a.state_out + ch * 3 * Q;
    uint8_t* bout = a.best_state ? a.best_state + ch * 3 * Q : nullptr;
    int32_t* hist = a.energy_hist ? a.energy_hist + ch * a.hist_stride : nullptr;
    uint8_t* rhist = a.rung_hist ? a.rung_hist + ch * a.hist_stride : nullptr;

    for (int w = lane; w < fw + bw; w += W) field[w] = 0;  // (field and occ are adjacent)
    int rung = a.rung_in ? min((int)a.rung_in[ch], R - 1) : slot;
    if (tl < R) {  // (a rung_in that is no permutation leaves a rung without a slot: it keeps this one, and nothing leaves the arrays)
        e_by_rung[tl] = 0;
        slot_by_rung[tl] = tl;
    }
    __syncthreads();
    if (lane == 0) {
        set_pad_bits(occ, bw, C);
        win[0] = win[1] = 0;
        red[0] = 0;  // "this chain repeats", until block_sum takes red
        rung_by_slot[slot] = rung;
    }
    __syncthreads();
    int rep = 0;
    for (int q = lane; q < Q; q += W) rep |= load_queen(queens, occ, in, N, q);
    if (rep) red[0] = 1;
    const bool held = __syncthreads_or(rep) != 0;  // (a barrier: queens and occ are complete, every byte of state_in is read)
    const bool repeated = red[0] != 0;
    store_queens(out, queens, Q, lane, W);  // the clamped input: what n_sweeps = 0 and a held ladder hand back
    if (bout) store_queens(bout, queens, Q, lane, W);

    if (held) {  // uniform over the workgroup: rule item 4
        int twoE = 0;
        for (int q = lane; q < Q; q += W) {
            const int p = queens[q];
            int n = 0;
            for (int o = 0; o < Q; o++) n += attacks(p, queens[o]);
            twoE += n - 1;  // itself
        }
        const int e = block_sum<W>(twoE, red, wave) >> 1;
        for (long long s = lane; s <= a.n_sweeps; s += W) {
            if (hist) hist[s] = e;
            if (rhist) rhist[s] = (uint8_t)rung;
        }
        if (lane == 0) {
            mcq_post::store_heatbath_figures(a, ch, e, e, e, 0, 0);
            if (a.flags) a.flags[ch] = (repeated ? MCQ_HEATBATH3D_REPEATED : 0) | MCQ_TEMPER3D_HELD;
            if (a.rung_out) a.rung_out[ch] = (uint8_t)rung;
            if (a.n_exchanges) a.n_exchanges[ch] = 0;
        }
        if (a.pair_accepted && tl < R - 1) a.pair_accepted[lad * (R - 1) + tl] = 0;
        return;
    }

    for (int x = lane; x < Q * SLOTS; x += W) put_slot<W, BITS, STEPS>(field, queens, N, x);
    __syncthreads();
    int twoE = 0;
    for (int q = lane; q < Q; q += W) twoE += attackers_at<BITS>(field, N, queens[q]);
    const int e_in = block_sum<W>(twoE, red, wave) >> 1;
    if (hist && lane == 0) hist[0] = e_in;
    if (rhist && lane == 0) rhist[0] = (uint8_t)rung;

    // this lane's run of field dwords: RUN is odd, so the lanes of an access group read 32 different banks
    const int RUN = ((fw + W - 1) / W) | 1;
    const int w0 = min(lane * RUN, fw), w1 = min(w0 + RUN, fw);
    const uint32_t seed = a.seeds[ch], seed0 = a.seeds[lad * R];
    int E = e_in, best = e_in;
    long long best_sweep = 0, changed = 0, exchanges = 0, accepted = 0;  // accepted: of pair tl, in the lanes tl < R - 1 of the ladder
    uint32_t rnd[4] = {0, 0, 0, 0};
    for (long long s = 0; s < a.n_sweeps; s++) {
        const uint32_t* row = a.table + s * R * D;
        for (int d = tl; d < R * D; d += LT) tab[d] = row[d];  // (its readers of the sweep before are behind that sweep's last barrier)
        const uint32_t* trow = tab + rung * D;
        const unsigned long long u0 = (unsigned long long)(a.first_sweep + s) * (unsigned long long)Q;
        for (int q = 0; q < Q; q++) {
            const int p = queens[q];
            const int pcell = cell_of(p, N);
            put<W, BITS, STEPS>(field, N, p, -1, lane, W, SLOTS);
            if (lane == 0) vacate(occ, pcell);
            __syncthreads();  // the field is a(q, .), the table rows are staged
            const int a_old = field_at<BITS>(field, pcell);
            uint32_t m = ~0u;
            for (int w = w0; w < w1; w++) {
                const uint32_t v = field[w];
                const uint32_t o = occ[(w * CPD) >> 5] >> ((w * CPD) & 31);
#pragma unroll
                for (int b = 0; b < CPD; b++)
                    if (!((o >> b) & 1u)) m = min(m, (v >> (b * BITS)) & MASK);
            }
            const int a_min = (int)block_min<W>(m, red, wave);
            uint32_t own = 0;
            for (int w = w0; w < w1; w++) {
                const uint32_t v = field[w];
                const uint32_t o = occ[(w * CPD) >> 5] >> ((w * CPD) & 31);
#pragma unroll
                for (int b = 0; b < CPD; b++)
                    if (!((o >> b) & 1u)) own += trow[min((int)((v >> (b * BITS)) & MASK) - a_min, D - 1)];
            }
            unsigned long long Wt;
            const unsigned long long before = block_scan<W>(own, scan, wave, Wt);
            const unsigned long long u = u0 + (unsigned)q;
            if ((u & 1) == 0 || q == 0) philox_block((uint32_t)(u >> 1), (uint32_t)(u >> 33), seed, 2u, rnd);
            const unsigned long long x = (u & 1) ? ((unsigned long long)rnd[3] << 32 | rnd[2]) : ((unsigned long long)rnd[1] << 32 | rnd[0]);
            const unsigned long long U = __umul64hi(x, Wt);
            if (own != 0 && before <= U && U < before + own) {  // one lane of the chain, as U < W: walk the run again to the smallest t with C_t > U
                unsigned long long c = before;
                bool found = false;
                for (int w = w0; w < w1 && !found; w++) {
                    const uint32_t v = field[w];
                    const uint32_t o = occ[(w * CPD) >> 5] >> ((w * CPD) & 31);
#pragma unroll
                    for (int b = 0; b < CPD; b++)
                        if (!found && !((o >> b) & 1u)) {
                            const int cnt = (int)((v >> (b * BITS)) & MASK);
                            c += trow[min(cnt - a_min, D - 1)];
                            if (c > U) {
                                win[0] = (uint32_t)(w * CPD + b), win[1] = (uint32_t)cnt;
                                found = true;
                            }
                        }
                }
            }
            __syncthreads();  // win is written; every lane has read queens[q] and the whole field before the queen goes back
            int t = p, tcell = pcell, a_new = a_old;
            if (Wt != 0) {  // (uniform over the chain, and no barrier inside.  W = 0: only a table with T[0] = 0; the queen stays)
                tcell = (int)win[0], a_new = (int)win[1];
                t = packed_of(tcell, N, N2);
            }
            E += a_new - a_old;
            changed += tcell != pcell;
            put<W, BITS, STEPS>(field, N, t, +1, lane, W, SLOTS);
            if (lane == 0) occupy(occ, queens, q, t, tcell);
            __syncthreads();
        }
        if (hist && lane == 0) hist[s + 1] = E;
        if (E < best) {
            best = E;
            best_sweep = s + 1;
            if (bout) store_queens(bout, queens, Q, lane, W);
        }
        const long long g1 = a.first_sweep + s + 1;
        if (g1 % a.every == 0) {  // uniform over the launch: the two barriers are met by every lane of the workgroup
            const long long ev = g1 / a.every - 1;
            if (lane == 0) {
                e_by_rung[rung] = E;
                slot_by_rung[rung] = slot;
            }
            __syncthreads();
            if (tl < R - 1 && ((tl ^ (int)ev) & 1) == 0) {
                const int sa = slot_by_rung[tl], sb = slot_by_rung[tl + 1];
                const uint32_t* X = a.swap_table + ((ev - a.events_before) * (R - 1) + tl) * (long long)a.swap_len;
                if (pair_swaps(e_by_rung[tl + 1] - e_by_rung[tl], X, a.swap_len, seed0, (unsigned long long)ev * (unsigned)R + (unsigned)tl)) {
                    rung_by_slot[sa] = tl + 1;
                    rung_by_slot[sb] = tl;
                    accepted++;
                }
            }
            __syncthreads();
            const int now = rung_by_slot[slot];
            exchanges += now != rung;
            rung = now;
        }
        if (rhist && lane == 0) rhist[s + 1] = (uint8_t)rung;
    }

    if (a.n_sweeps > 0) store_queens(out, queens, Q, lane, W);
    if (lane == 0) {
        mcq_post::store_heatbath_figures(a, ch, e_in, E, best, best_sweep, changed);
        if (a.flags) a.flags[ch] = 0;
        if (a.rung_out) a.rung_out[ch] = (uint8_t)rung;
        if (a.n_exchanges) a.n_exchanges[ch] = exchanges;
    }
    if (a.pair_accepted && tl < R - 1) a.pair_accepted[lad * (R - 1) + tl] = accepted;
}

// ---- shapes ----
// lanes per chain: the W of mcq_field::for_shape_of(N), as far as R chains fit the 1024 lanes of a workgroup
int chain_lanes(int N, int R) { return std::min(N <= 12 ? 64 : N <= 19 ? 256 : 1024, 1024 / R); }
int field_bits(int N) { return N <= 19 ? 8 : 16; }

// dwords of one chain region, a multiple of 4 (a region's scan stays 8-byte aligned, the staged rows 16)
long long chain_words(int N, int Q) {
    const long long cells = (long long)N * N * N, cpd = 32 / field_bits(N);
    return (HDR + (cells + cpd - 1) / cpd + (cells + 31) / 32 + (Q + 1) / 2 + 3) / 4 * 4;
}

long long ladder_bytes(int N, int R, int Q, int D) { return 4 * (R * chain_words(N, Q) + (long long)R * D + 3 * R); }

// the cells whose weights a lane adds up in 32 bits before the sum goes to 64
long long lane_cells(int N, int R) {
    const long long cells = (long long)N * N * N, cpd = 32 / field_bits(N), fw = (cells + cpd - 1) / cpd, W = chain_lanes(N, R);
    return (((fw + W - 1) / W) | 1) * cpd;
}

long long events_of(long long first, long long n, long long K) { return (first + n) / K - first / K; }

// what both entry points refuse of the shape of a call
int check_temper3d(const mcq_temper3d* q) {
    if (!q) return fail(g_temper3d_err, MCQ_EINVAL, "mcq_temper3d: NULL parameter block");
    const int rc = mcq_post::check_full3d(g_temper3d_err, "tempered heat-bath sweep", q->N, q->n_queens, (long long)q->n_chains);
    if (rc != MCQ_OK) return rc;
    const long long R = (long long)q->replicas, K = (long long)q->exchange_every;
    if (R != 2 && R != 4 && R != 8 && R != 16) return fail(g_temper3d_err, MCQ_EINVAL, "replicas must be 2, 4, 8 or 16, got %lld", R);
    if (q->n_chains % R) return fail(g_temper3d_err, MCQ_EINVAL, "replicas (%lld) must divide n_chains (%lld)", R, (long long)q->n_chains);
    if (q->n_sweeps < 0) return fail(g_temper3d_err, MCQ_EINVAL, "n_sweeps must be >= 0, got %lld", (long long)q->n_sweeps);
    if (q->first_sweep < 0) return fail(g_temper3d_err, MCQ_EINVAL, "first_sweep must be >= 0, got %lld", (long long)q->first_sweep);
    const uint64_t end = (uint64_t)q->first_sweep + (uint64_t)q->n_sweeps, Q = (uint64_t)queens_of(q);
    if (end > ((1ull << 62) - 1) / Q)
        return fail(g_temper3d_err, MCQ_EINVAL, "first_sweep + n_sweeps = %llu: the update index (first_sweep + n_sweeps) Q must stay below 2^62", (unsigned long long)end);
    if (K < 1) return fail(g_temper3d_err, MCQ_EINVAL, "exchange_every must be >= 1, got %lld", K);
    if (end / (uint64_t)K > (uint64_t)INT64_MAX / (uint64_t)R)
        return fail(g_temper3d_err, MCQ_EINVAL, "exchange_every = %lld: the word index of the exchange stream, events times replicas, must stay below 2^63", K);
    const long long events = events_of((long long)q->first_sweep, (long long)q->n_sweeps, K);
    if (q->n_events != events)
        return fail(g_temper3d_err, MCQ_EINVAL, "n_events must be floor((first_sweep + n_sweeps) / exchange_every) - floor(first_sweep / exchange_every) = %lld, got %lld",
                    events, (long long)q->n_events);
    if (q->table_len < 1 || q->table_len > MCQ_MAX_HEATBATH_TABLE)
        return fail(g_temper3d_err, MCQ_EINVAL, "table_len out of range [1, %d]: %lld", MCQ_MAX_HEATBATH_TABLE, (long long)q->table_len);
    if (q->swap_len < 1 || q->swap_len > MCQ_MAX_TEMPER_SWAP_TABLE)
        return fail(g_temper3d_err, MCQ_EINVAL, "swap_len out of range [1, %d]: %lld", MCQ_MAX_TEMPER_SWAP_TABLE, (long long)q->swap_len);
    return MCQ_OK;
}

// ... and of its pointers, behind the shape: mcq_temper3d_device puts the LDS limit between the two, so a shape is judged before a buffer
int check_temper3d_buffers(const mcq_temper3d* q) {
    if (!q->seeds) return fail(g_temper3d_err, MCQ_EINVAL, "seeds is required");
    if (!q->table && q->n_sweeps > 0) return fail(g_temper3d_err, MCQ_EINVAL, "table is required (n_sweeps x replicas rows of table_len words)");
    if (!q->swap_table && q->n_events > 0) return fail(g_temper3d_err, MCQ_EINVAL, "swap_table is required (n_events x (replicas - 1) rows of swap_len words)");
    if (!q->state_in) return fail(g_temper3d_err, MCQ_EINVAL, "state_in is required");
    if (!q->state_out) return fail(g_temper3d_err, MCQ_EINVAL, "state_out is required");
    if ((q->energy_hist || q->rung_hist) && q->hist_stride < q->n_sweeps + 1)
        return fail(g_temper3d_err, MCQ_EINVAL, "hist_stride must be >= n_sweeps + 1 = %lld, got %lld", (long long)q->n_sweeps + 1, (long long)q->hist_stride);
    return MCQ_OK;
}

// what the host entry point refuses on top of that: it reads the table and the rungs, which the device entry point cannot
int check_temper3d_inputs(const mcq_temper3d* q) {
    const long long D = (long long)q->table_len, R = (long long)q->replicas;
    for (long long s = 0; s < q->n_sweeps; s++)
        for (long long t = 0; t < R; t++)
            for (long long d = 0; d < D; d++)
                if (q->table[(s * R + t) * D + d] > (1u << MCQ_HEATBATH_WEIGHT_BITS))
                    return fail(g_temper3d_err, MCQ_EINVAL, "table: the entry of sweep %lld, rung %lld at index %lld is %u, above 2^%d (a lane sums up to 255 entries in 32 bits)",
                                s, t, d, (unsigned)q->table[(s * R + t) * D + d], MCQ_HEATBATH_WEIGHT_BITS);
    if (q->rung_in)
        for (long long g = 0; g < q->n_chains / R; g++) {
            unsigned seen = 0;
            for (long long r = 0; r < R; r++) {
                const int t = q->rung_in[g * R + r];
                if (t >= R || (seen >> t & 1u))
                    return fail(g_temper3d_err, MCQ_EINVAL, "rung_in: the rungs of ladder %lld are no permutation of 0 .. %lld (slot %lld holds %d)", g, R - 1, r, t);
                seen |= 1u << t;
            }
        }
    return MCQ_OK;
}

template <int W, int BITS, int STEPS>
hipError_t launch_temper3d(const Temper3dArgs& a, long long n_ladders, size_t bytes, hipStream_t s) {
    if (bytes > 32 * 1024) {  // (the default limit is 64 KiB; a ladder takes up to 160)
        const hipError_t e = hipFuncSetAttribute((const void*)mcq_temper3d_kernel<W, BITS, STEPS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((mcq_temper3d_kernel<W, BITS, STEPS>), dim3((unsigned)n_ladders), dim3(a.R * W), bytes, s, a);
    return hipGetLastError();
}

// one sweep of one chain on the host with the row T: the body of mcq_heatbath3d_host's sweep, E and n_changed moved
void host_sweep(HostField& f, int D, const uint32_t* T, uint64_t u0, uint32_t seed, int& E, long long& changed) {
    const std::vector<int>& S = f.S;
    const std::vector<uint8_t>& occ = f.occ;
    const int C = f.C;
    for (int n = 0; n < f.Q; n++) {
        const int p = f.pos[(size_t)n];
        f.take_out(n);
        int a_min = INT_MAX;
        for (int c = 0; c < C; c++)
            if (!occ[(size_t)c] && S[(size_t)c] < a_min) a_min = S[(size_t)c];
        uint64_t Wt = 0;
        for (int c = 0; c < C; c++)
            if (!occ[(size_t)c]) Wt += T[std::min(S[(size_t)c] - a_min, D - 1)];
        const uint64_t u = u0 + (uint64_t)n;
        uint32_t r[4];
        philox_block((uint32_t)(u >> 1), (uint32_t)(u >> 33), seed, 2u, r);
        const uint64_t x = (u & 1) ? ((uint64_t)r[3] << 32 | r[2]) : ((uint64_t)r[1] << 32 | r[0]);
        const uint64_t U = (uint64_t)(((unsigned __int128)x * Wt) >> 64);
        int t = p;
        if (Wt != 0) {
            uint64_t c_sum = 0;
            for (int c = 0; c < C; c++) {
                if (occ[(size_t)c]) continue;
                c_sum += T[std::min(S[(size_t)c] - a_min, D - 1)];
                if (c_sum > U) {
                    t = c;
                    break;
                }
            }
        }
        E += S[(size_t)t] - S[(size_t)p];
        changed += t != p;
        f.put_back(n, t);
    }
}

// ladders first .. last - 1 through the rule, one HostField per slot
void host_ladders(const mcq_temper3d* q, long long first, long long last) {
    const int N = q->N, Q = queens_of(q), D = (int)q->table_len, R = (int)q->replicas, DX = (int)q->swap_len;
    const long long K = (long long)q->exchange_every, before = (long long)q->first_sweep / K;
    std::vector<HostField> f((size_t)R, HostField(N, Q));
    std::vector<int> E((size_t)R), e_in((size_t)R), best((size_t)R), rung((size_t)R), by_rung((size_t)R), repeated((size_t)R);
    std::vector<long long> best_sweep((size_t)R), changed((size_t)R), exchanges((size_t)R), accepted((size_t)R);
    for (long long g = first; g < last; g++) {
        const long long c0 = g * R;
        bool held = false;
        for (int r = 0; r < R; r++) {
            const long long ch = c0 + r;
            repeated[r] = f[r].load(q->state_in + ch * 3 * Q);
            held |= repeated[r] != 0;
            E[r] = e_in[r] = best[r] = f[r].energy();
            best_sweep[r] = changed[r] = exchanges[r] = accepted[r] = 0;
            rung[r] = q->rung_in ? q->rung_in[ch] : r;
            if (q->energy_hist) q->energy_hist[ch * q->hist_stride] = E[r];
            if (q->rung_hist) q->rung_hist[ch * q->hist_stride] = (uint8_t)rung[r];
            if (q->best_state) f[r].store(q->best_state + ch * 3 * Q);
        }
        const uint32_t seed0 = q->seeds[c0];
        for (long long s = 0; s < q->n_sweeps; s++) {
            if (held) {  // rule item 4: nothing moves, every history entry is constant
                for (int r = 0; r < R; r++) {
                    if (q->energy_hist) q->energy_hist[(c0 + r) * q->hist_stride + s + 1] = E[r];
                    if (q->rung_hist) q->rung_hist[(c0 + r) * q->hist_stride + s + 1] = (uint8_t)rung[r];
                }
                continue;
            }
            const uint64_t u0 = (uint64_t)(q->first_sweep + s) * (uint64_t)Q;
            for (int r = 0; r < R; r++) {
                const long long ch = c0 + r;
                host_sweep(f[r], D, q->table + (s * R + rung[r]) * D, u0, q->seeds[ch], E[r], changed[r]);
                if (q->energy_hist) q->energy_hist[ch * q->hist_stride + s + 1] = E[r];
                if (E[r] < best[r]) {
                    best[r] = E[r];
                    best_sweep[r] = s + 1;
                    if (q->best_state) f[r].store(q->best_state + ch * 3 * Q);
                }
            }
            const long long g1 = q->first_sweep + s + 1;
            if (g1 % K == 0) {
                const long long ev = g1 / K - 1;
                for (int r = 0; r < R; r++) by_rung[rung[r]] = r;
                for (int t = (int)(ev & 1); t + 1 < R; t += 2) {
                    const int sa = by_rung[t], sb = by_rung[t + 1];
                    const uint32_t* X = q->swap_table + ((ev - before) * (R - 1) + t) * (long long)DX;
                    if (pair_swaps(E[sb] - E[sa], X, DX, seed0, (unsigned long long)ev * (unsigned)R + (unsigned)t)) {
                        rung[sa] = t + 1, rung[sb] = t;
                        exchanges[sa]++, exchanges[sb]++, accepted[t]++;
                    }
                }
            }
            if (q->rung_hist)
                for (int r = 0; r < R; r++) q->rung_hist[(c0 + r) * q->hist_stride + s + 1] = (uint8_t)rung[r];
        }
        for (int r = 0; r < R; r++) {
            const long long ch = c0 + r;
            f[r].store(q->state_out + ch * 3 * Q);
            mcq_post::store_heatbath_figures(*q, ch, e_in[r], E[r], best[r], best_sweep[r], changed[r]);
            if (q->flags) q->flags[ch] = held ? (repeated[r] ? MCQ_HEATBATH3D_REPEATED : 0) | MCQ_TEMPER3D_HELD : 0;
            if (q->rung_out) q->rung_out[ch] = (uint8_t)rung[r];
            if (q->n_exchanges) q->n_exchanges[ch] = exchanges[r];
            if (q->pair_accepted && r < R - 1) q->pair_accepted[g * (R - 1) + r] = accepted[r];
        }
    }
}

}  // namespace

extern "C" {

const char* mcq_temper3d_last_error(void) { return g_temper3d_err; }

int mcq_temper3d_host(const mcq_temper3d* q) {
    int rc = check_temper3d(q);
    if (rc == MCQ_OK) rc = check_temper3d_buffers(q);
    if (rc == MCQ_OK) rc = check_temper3d_inputs(q);
    if (rc != MCQ_OK) return rc;
    mcq_post::for_chains(q->n_chains / q->replicas, [q](long long first, long long last) { host_ladders(q, first, last); });
    return MCQ_OK;
}

int mcq_temper3d_device(const mcq_temper3d* q, void* hip_stream) {
    int rc = check_temper3d(q);
    if (rc != MCQ_OK) return rc;
    const int N = q->N, R = (int)q->replicas, D = (int)q->table_len, Q = queens_of(q);
    const long long bytes = ladder_bytes(N, R, Q, D);
    if (bytes > MCQ_MAX_TEMPER_LDS - MCQ_TEMPER3D_STATIC_LDS)
        return fail(g_temper3d_err, MCQ_EINVAL, "N = %d with replicas = %d and n_queens = %d: a ladder takes %lld bytes of LDS, above the %d of a workgroup "
                    "(include/mcq.h tabulates what fits; mcq_temper3d_host runs every shape)", N, R, Q, bytes, MCQ_MAX_TEMPER_LDS - MCQ_TEMPER3D_STATIC_LDS);
    if (lane_cells(N, R) > 255)
        return fail(g_temper3d_err, MCQ_EINVAL, "N = %d with replicas = %d: a lane would add up the weights of %lld cells in 32 bits, above 255", N, R, lane_cells(N, R));
    rc = check_temper3d_buffers(q);
    if (rc != MCQ_OK) return rc;
    const Temper3dArgs a{q->seeds, q->table, q->swap_table, q->rung_in, q->rung_out, q->state_in, q->state_out, q->energy_in, q->energy_out, q->best_energy,
                         q->best_sweep, q->best_state, q->n_changed, q->energy_hist, q->n_exchanges, q->rung_hist, q->pair_accepted, q->flags,
                         (long long)q->hist_stride, (long long)q->n_sweeps, (long long)q->first_sweep, (long long)q->exchange_every,
                         (long long)(q->first_sweep / q->exchange_every), D, (int)q->swap_len, R, (int)chain_words(N, Q), N, Q};
    hipStream_t s = (hipStream_t)hip_stream;
    const long long n_ladders = (long long)(q->n_chains / R);
    const int W = chain_lanes(N, R);
    hipError_t e;
    if (N <= 12) e = launch_temper3d<64, 8, 32>(a, n_ladders, (size_t)bytes, s);
    else if (N <= 19) e = W == 256 ? launch_temper3d<256, 8, 64>(a, n_ladders, (size_t)bytes, s)
                      : W == 128 ? launch_temper3d<128, 8, 64>(a, n_ladders, (size_t)bytes, s)
                                 : launch_temper3d<64, 8, 64>(a, n_ladders, (size_t)bytes, s);
    else if (W == 512) e = launch_temper3d<512, 16, 64>(a, n_ladders, (size_t)bytes, s);
    else if (W == 256) e = launch_temper3d<256, 16, 64>(a, n_ladders, (size_t)bytes, s);
    else if (W == 128) e = launch_temper3d<128, 16, 64>(a, n_ladders, (size_t)bytes, s);
    else return fail(g_temper3d_err, MCQ_EINVAL, "N = %d with replicas = %d: no instantiation (a ladder of 16 beyond N = 19 does not fit the LDS)", N, R);
    if (e != hipSuccess) return fail(g_temper3d_err, MCQ_EDEVICE, "mcq_temper3d_device: %s", hipGetErrorString(e));
    return MCQ_OK;
}

}  // extern "C"
