// mcq_temper.hip -- parallel tempering of board heat-bath sweeps, one ladder per workgroup (include/mcq.h: mcq_temper, where the rule is
// stated).  The sweep is that of csrc/mcq_heatbath.hip; what is new is that the R replicas of a ladder sit in ONE workgroup, each at the
// table row of its rung, and trade rungs between sweeps through LDS, so that a whole tempered run is one launch.
//
//   kernel  the column update is mcq_heatbath_kernel's, with its instantiations for N <= 64: the lanes of a GROUP (16, 32 or 64) are the
//           candidate heights of one column, the chain keeps four copies of its heights in LDS, one per line family, the minimum and the
//           prefix sum run with DPP, the selection is a ballot, one Philox block serves four columns.  A chain still lives inside one
//           wavefront, and a changed height is stored by every lane of its group, so each lane's later reads are ordered behind its own
//           store by program order, as there.  The lane helpers (group_min, group_scan, line_hits) are shared: csrc/mcq_columns.h.
//           A WORKGROUP is one ladder: R GW lanes, 1 to 16 wavefronts; where a ladder is narrower than a wavefront (R = 2 at N <= 16)
//           a workgroup holds two, and a ladder beyond the last one walks the last ladder and writes nothing.  Dynamic LDS per ladder:
//           the R chain regions (6 NP^2 bytes each), the sweep's R table rows, staged once per sweep (R D dwords), and 3 R words for
//           the event: energy by rung, slot by rung, rung by slot.
//           An EVENT: lane 0 of each chain posts its energy and its slot under its rung; barrier; lane t of the ladder decides pair t
//           (X comes from global memory: an event is rare), writes the two new rungs and counts the accept in a register it keeps for
//           the whole kernel; barrier; every chain reads its rung back.  Every barrier sits in control flow that is uniform over the
//           workgroup: the sweep count is the launch's, and "is this sweep followed by an event" depends on g and K alone.
//   counter form (N <= MCQ_MAX_N_TEMPER_COUNTERS, mcq_temper_counters_device): mcq_temper_counters_kernel is the same ladder with the
//           column update of mcq_heatbath_counters_kernel -- per chain the byte counters of the cube's 12 line families and one copy of
//           the heights (csrc/mcq_columns.h: counter_offset, counter_region_bytes), 12 byte reads per height, 24 LDS atomics where a
//           drawn height differs.  16 lanes per chain for every N; instantiated per (padding, R) with the launch bounds of its real
//           workgroup (64, 64, 128 or 256 lanes), which the 1 024 of the kernel above would cap at 128 VGPRs.  A slot's counters stay
//           with the slot at an exchange: only the rung moves.
//   host    mcq_temper_host: the same rule over host buffers, ladder by ladder.
//
// Built for gfx950 only, with csrc/mcq_hip.hip:  hipcc --offload-arch=gfx950 -O3 -ffp-contract=off
#include <hip/hip_runtime.h>

#include <climits>
#include <vector>

#include "../../include/mcq.h"
#include "mcq_columns.h"
#include "mcq_post.h"

namespace {

using mcq_columns::counter_offset;
using mcq_columns::group_min;
using mcq_columns::group_scan;
using mcq_columns::line_hits;
using mcq_post::fail;
using mcq_post::host_counts;
using mcq_post::philox_block;

thread_local char g_temper_err[256] = "";

struct TemperArgs {
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
    long long hist_stride;
    long long n_ladders;
    long long n_sweeps;
    long long first_sweep;
    long long every;       // K
    long long events_before;  // floor(first_sweep / K)
    int table_len;
    int swap_len;
    int R;
    int ladder_words;      // dwords of LDS per ladder
    int N;
};

// word w of the exchange stream of a ladder whose slot 0 is seeded `seed`: key word 3
__host__ __device__ __forceinline__ uint32_t exchange_word(uint32_t seed, unsigned long long w) {
    uint32_t r[4];
    philox_block((uint32_t)(w >> 2), (uint32_t)(w >> 34), seed, 3u, r);
    const int e = (int)(w & 3);
    return e == 0 ? r[0] : e == 1 ? r[1] : e == 2 ? r[2] : r[3];
}

// rule item 3 for one pair: Delta = E_b - E_a, X = the pair's row of the event
__host__ __device__ __forceinline__ bool pair_swaps(int delta, const uint32_t* X, int DX, uint32_t seed0, unsigned long long w) {
    if (delta >= 0) return true;
    const long long d = -(long long)delta;
    return exchange_word(seed0, w) < X[d < DX - 1 ? d : DX - 1];
}

// threads of a workgroup: one ladder of R chains of GW lanes, two ladders where that is half a wavefront
__host__ __device__ constexpr int temper_threads(int R, int GW) { return R * GW < 64 ? 64 : R * GW; }

template <int GW, int NP>
__global__ __launch_bounds__(1024) void mcq_temper_kernel(TemperArgs a) {
    constexpr int NPW = NP / 4;        // dwords per line
    constexpr int FAM = NP * NPW;      // dwords of the row copy (and of the column copy); the two diagonal copies take 2 FAM each
    constexpr int CHAIN = 6 * FAM;
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const int N = a.N, Q = N * N, D = a.table_len, R = a.R;
    const int LT = R * GW;                                   // lanes of a ladder
    const int lane = threadIdx.x & (GW - 1);
    const int wgrp = (threadIdx.x & 63) / GW;                // the group's place in its wavefront
    const int lib = threadIdx.x / LT;                        // ladder in the workgroup (0, or 0 / 1 where two share it)
    const int tl = threadIdx.x - lib * LT;                   // lane of the ladder
    const int slot = tl / GW;                                // chain of the ladder
    const long long ladder = (long long)blockIdx.x * (blockDim.x / LT) + lib;
    const bool valid = ladder < a.n_ladders;
    const long long lad = valid ? ladder : a.n_ladders - 1;  // a ladder beyond the last one walks the last ladder and writes nothing
    const long long ch = lad * R + slot;
    uint32_t* lbase = lds + lib * a.ladder_words;
    uint32_t* base = lbase + slot * CHAIN;
    uint32_t* tab = lbase + R * CHAIN;                       // [R][D]: the sweep's rows by rung
    int* e_by_rung = (int*)(tab + R * D);
    int* slot_by_rung = e_by_rung + R;
    int* rung_by_slot = slot_by_rung + R;
    uint8_t* rows = (uint8_t*)base;
    uint8_t* cols = rows + 4 * FAM;
    uint8_t* diag = rows + 8 * FAM;
    uint8_t* anti = rows + 16 * FAM;
    for (int w = lane; w < CHAIN; w += GW) base[w] = 0xFFFFFFFFu;
    int rung = a.rung_in ? min((int)a.rung_in[ch], R - 1) : slot;
    if (tl < R) {  // (a rung_in that is no permutation leaves a rung without a slot: it keeps this one, and nothing leaves the arrays)
        e_by_rung[tl] = 0;
        slot_by_rung[tl] = tl;
    }
    if (lane == 0) rung_by_slot[slot] = rung;
    __syncthreads();
    const uint8_t* in = a.state_in + ch * Q;
    for (int c = lane; c < Q; c += GW) {
        const int v = in[c], i = c / N, j = c - i * N;
        const uint8_t hv = (uint8_t)(v < N ? v : N - 1);
        rows[i * NP + j] = hv;
        cols[j * NP + i] = hv;
        diag[(i - j + N - 1) * NP + i] = hv;
        anti[(i + j) * NP + i] = hv;
    }
    __syncthreads();
    if (valid && a.best_state) {  // until a sweep end is strictly lower: the (clamped) input
        uint8_t* out = a.best_state + ch * Q;
        for (int c = lane; c < Q; c += GW) {
            const int i = c / N;
            out[c] = rows[i * NP + (c - i * N)];
        }
    }
    const int k0 = lane;
    const uint32_t seed = a.seeds[ch], seed0 = a.seeds[lad * R];
    int32_t* hist = a.energy_hist ? a.energy_hist + ch * a.hist_stride : nullptr;
    uint8_t* rhist = a.rung_hist ? a.rung_hist + ch * a.hist_stride : nullptr;
    if (valid && rhist && lane == 0) rhist[0] = (uint8_t)rung;

    int E = 0, e_in = 0, best = 0;
    long long best_sweep = 0, changed = 0, exchanges = 0, accepted = 0;  // accepted: of pair tl, in the lanes tl < R - 1 of a ladder
    uint32_t rnd[4] = {0, 0, 0, 0};
    // sweep -1 is the recount of the input: the same walk with no update
    for (long long s = -1; s < a.n_sweeps; s++) {
        const bool recount = s < 0;
        if (!recount) {
            __syncthreads();
            const uint32_t* row = a.table + s * R * D;
            for (int d = tl; d < R * D; d += LT) tab[d] = row[d];
            __syncthreads();
        }
        const uint32_t* trow = tab + rung * D;
        const unsigned long long w0 = recount ? 0ull : (unsigned long long)(a.first_sweep + s) * (unsigned long long)Q;
        int twoE = 0;
        for (int i = 0, c = 0; i < N; i++)
            for (int j = 0; j < N; j++, c++) {
                int c0 = 0, c1 = 0;  // (c1: the second height of a lane beyond N = 64, which no ladder reaches)
                const int dl = i - j + N - 1, al = i + j;
                line_hits<1, NP>(base + i * NPW, j, k0, 0, c0, c1);
                line_hits<1, NP>(base + FAM + j * NPW, i, k0, 0, c0, c1);
                line_hits<1, NP>(base + 2 * FAM + dl * NPW, i, k0, 0, c0, c1);
                line_hits<1, NP>(base + 4 * FAM + al * NPW, i, k0, 0, c0, c1);
                const int cur = rows[i * NP + j];
                c0 -= k0 == cur ? 4 : 0;
                const int a_old = __shfl(c0, cur & (GW - 1), GW);
                if (recount) {
                    twoE += a_old;
                    continue;
                }
                const int a_min = group_min<GW>(k0 < N ? c0 : INT_MAX);
                const uint32_t wt0 = k0 < N ? trow[k0 < N ? min(c0 - a_min, D - 1) : 0] : 0u;
                uint32_t W;
                const uint32_t C0 = group_scan<GW>(wt0, lane, W);
                const unsigned long long w = w0 + (unsigned)c;
                if ((w & 3) == 0 || c == 0) philox_block((uint32_t)(w >> 2), (uint32_t)(w >> 34), seed, 1u, rnd);
                const int e = (int)(w & 3);
                const uint32_t x = e == 0 ? rnd[0] : e == 1 ? rnd[1] : e == 2 ? rnd[2] : rnd[3];
                const uint32_t U = __umulhi(x, W);
                // the smallest k with C_k > U = the number of heights with C_k <= U (C is non-decreasing; a lane beyond N holds W > U)
                const unsigned long long gmask = GW == 64 ? ~0ull : ((1ull << GW) - 1);
                int kn = __popcll((__ballot(C0 <= U) >> (wgrp * GW)) & gmask);
                kn = min(kn, N - 1);  // (only a table with T[0] = 0, W = 0, gets here: the last height, as in the host code)
                const int a_new = __shfl(c0, kn & (GW - 1), GW);
                E += a_new - a_old;
                changed += kn != cur;
                const uint8_t hv = (uint8_t)kn;
                rows[i * NP + j] = hv;
                cols[j * NP + i] = hv;
                diag[dl * NP + i] = hv;
                anti[al * NP + i] = hv;
            }
        if (recount) {
            E = e_in = best = twoE >> 1;
            if (valid && hist && lane == 0) hist[0] = E;
            continue;
        }
        if (valid && hist && lane == 0) hist[s + 1] = E;
        if (E < best) {
            best = E;
            best_sweep = s + 1;
            if (valid && a.best_state) {
                uint8_t* out = a.best_state + ch * Q;
                for (int c = lane; c < Q; c += GW) {
                    const int i = c / N;
                    out[c] = rows[i * NP + (c - i * N)];
                }
            }
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
        if (valid && rhist && lane == 0) rhist[s + 1] = (uint8_t)rung;
    }
    if (!valid) return;
    uint8_t* out = a.state_out + ch * Q;
    for (int c = lane; c < Q; c += GW) {
        const int i = c / N;
        out[c] = rows[i * NP + (c - i * N)];
    }
    if (lane == 0) {
        mcq_post::store_heatbath_figures(a, ch, e_in, E, best, best_sweep, changed);
        if (a.rung_out) a.rung_out[ch] = (uint8_t)rung;
        if (a.n_exchanges) a.n_exchanges[ch] = exchanges;
    }
    if (a.pair_accepted && tl < R - 1) a.pair_accepted[lad * (R - 1) + tl] = accepted;
}

// ---- the counter form, N <= MCQ_MAX_N_TEMPER_COUNTERS (include/mcq.h: mcq_temper_counters_device) ----
// The ladder of mcq_temper_kernel -- the R rows staged per sweep, the row of the slot's rung, the event's two barriers and three arrays,
// pair_accepted in registers, the ladder beyond the last one -- around the column update of mcq_heatbath_counters_kernel
// (csrc/mcq_heatbath.hip, where the counters are explained).  Dynamic LDS per ladder: the R counter regions, the R D dwords of rows and
// 3 R words for the event.  A chain's region is touched by the 16 lanes of its group alone, which sit in one wavefront, so the update's
// atomics need no barrier: the branch on "changed" holds none, and every barrier is where mcq_temper_kernel has it.
template <int NP, int R>
__global__ __launch_bounds__(temper_threads(R, 16)) void mcq_temper_counters_kernel(TemperArgs a) {
    constexpr int GW = 16, LT = R * GW;                               // lanes of a chain, lanes of a ladder
    constexpr int CNT = mcq_columns::counter_bytes(NP);               // bytes of counters; a multiple of 4 for NP = 8, 12, 16
    constexpr int CHAIN = mcq_columns::counter_region_bytes(NP);      // bytes of a chain's region: >= CNT + NP^2, = 64 mod 128
    static_assert(CNT % 4 == 0 && NP <= GW, "counter layout");
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const int N = a.N, Q = N * N, D = a.table_len;
    const int lane = threadIdx.x & (GW - 1);
    const int wgrp = (threadIdx.x & 63) / GW;                // the group's place in its wavefront
    const int lib = threadIdx.x / LT;                        // ladder in the workgroup (0, or 0 / 1 where two share it: R = 2)
    const int tl = threadIdx.x - lib * LT;                   // lane of the ladder
    const int slot = tl / GW;                                // chain of the ladder
    const long long ladder = (long long)blockIdx.x * (temper_threads(R, GW) / LT) + lib;
    const bool valid = ladder < a.n_ladders;
    const long long lad = valid ? ladder : a.n_ladders - 1;  // a ladder beyond the last one walks the last ladder and writes nothing
    const long long ch = lad * R + slot;
    uint32_t* lbase = lds + lib * a.ladder_words;
    uint32_t* cw = lbase + slot * (CHAIN / 4);
    const uint8_t* cb = (const uint8_t*)cw;
    uint8_t* hts = (uint8_t*)cw + CNT;
    uint32_t* tab = lbase + R * (CHAIN / 4);                 // [R][D]: the sweep's rows by rung
    int* e_by_rung = (int*)(tab + R * D);
    int* slot_by_rung = e_by_rung + R;
    int* rung_by_slot = slot_by_rung + R;
    for (int w = lane; w < CNT / 4; w += GW) cw[w] = 0u;
    int rung = a.rung_in ? min((int)a.rung_in[ch], R - 1) : slot;
    if (tl < R) {  // (a rung_in that is no permutation leaves a rung without a slot: it keeps this one, and nothing leaves the arrays)
        e_by_rung[tl] = 0;
        slot_by_rung[tl] = tl;
    }
    if (lane == 0) rung_by_slot[slot] = rung;
    __syncthreads();
    const uint8_t* in = a.state_in + ch * Q;
    for (int c = lane; c < Q; c += GW) {
        const int v = in[c], i = c / N, j = c - i * N;
        const int hv = v < N ? v : N - 1;
        hts[c] = (uint8_t)hv;
#pragma unroll
        for (int f = 0; f < 12; f++) {
            const int b = counter_offset(f / 3, f % 3, i, j, N) + hv;
            atomicAdd(cw + (b >> 2), 1u << (8 * (b & 3)));
        }
    }
    __syncthreads();
    if (valid && a.best_state) {  // until a sweep end is strictly lower: the (clamped) input
        uint8_t* out = a.best_state + ch * Q;
        for (int c = lane; c < Q; c += GW) out[c] = hts[c];
    }
    const int k0 = lane, kr = min(lane, N - 1);  // a lane beyond N reads the counters of the last height and is left out below
    const int own_dir = lane / 3, own_step = lane - 3 * own_dir;  // lane f < 12 updates family f
    const uint32_t seed = a.seeds[ch], seed0 = a.seeds[lad * R];
    int32_t* hist = a.energy_hist ? a.energy_hist + ch * a.hist_stride : nullptr;
    uint8_t* rhist = a.rung_hist ? a.rung_hist + ch * a.hist_stride : nullptr;
    if (valid && rhist && lane == 0) rhist[0] = (uint8_t)rung;

    int E = 0, e_in = 0, best = 0;
    long long best_sweep = 0, changed = 0, exchanges = 0, accepted = 0;  // accepted: of pair tl, in the lanes tl < R - 1 of a ladder
    uint32_t rnd[4] = {0, 0, 0, 0};
    // sweep -1 is the recount of the input: the same walk with no update
    for (long long s = -1; s < a.n_sweeps; s++) {
        const bool recount = s < 0;
        if (!recount) {
            __syncthreads();
            const uint32_t* row = a.table + s * R * D;
            for (int d = tl; d < R * D; d += LT) tab[d] = row[d];
            __syncthreads();
        }
        const uint32_t* trow = tab + rung * D;
        const unsigned long long w0 = recount ? 0ull : (unsigned long long)(a.first_sweep + s) * (unsigned long long)Q;
        int twoE = 0;
        for (int i = 0, c = 0; i < N; i++)
            for (int j = 0; j < N; j++, c++) {
                int c0 = 0;
#pragma unroll
                for (int f = 0; f < 12; f++) c0 += cb[counter_offset(f / 3, f % 3, i, j, N) + kr];
                const int cur = hts[c];
                c0 -= k0 == cur ? 12 : 0;
                const int a_old = __shfl(c0, cur, GW);
                if (recount) {
                    twoE += a_old;
                    continue;
                }
                const int a_min = group_min<GW>(k0 < N ? c0 : INT_MAX);
                const uint32_t wt0 = k0 < N ? trow[min(c0 - a_min, D - 1)] : 0u;
                uint32_t W;
                const uint32_t C0 = group_scan<GW>(wt0, lane, W);
                const unsigned long long w = w0 + (unsigned)c;
                if ((w & 3) == 0 || c == 0) philox_block((uint32_t)(w >> 2), (uint32_t)(w >> 34), seed, 1u, rnd);
                const int e = (int)(w & 3);
                const uint32_t x = e == 0 ? rnd[0] : e == 1 ? rnd[1] : e == 2 ? rnd[2] : rnd[3];
                const uint32_t U = __umulhi(x, W);
                // the smallest k with C_k > U = the number of heights with C_k <= U (C is non-decreasing; a lane beyond N holds W > U)
                int kn = __popcll((__ballot(C0 <= U) >> (wgrp * GW)) & ((1ull << GW) - 1));
                kn = min(kn, N - 1);  // (only a table with T[0] = 0, W = 0, gets here: the last height, as in the host code)
                const int a_new = __shfl(c0, kn, GW);
                E += a_new - a_old;
                changed += kn != cur;
                if (kn != cur && lane < 12) {
                    const int o = counter_offset(own_dir, own_step, i, j, N);
                    const int b0 = o + cur, b1 = o + kn;
                    atomicSub(cw + (b0 >> 2), 1u << (8 * (b0 & 3)));
                    atomicAdd(cw + (b1 >> 2), 1u << (8 * (b1 & 3)));
                }
                hts[c] = (uint8_t)kn;  // by every lane of the group: same address, same value
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // (no instruction: the compiler keeps the next column's reads behind the updates)
            }
        if (recount) {
            E = e_in = best = twoE >> 1;
            if (valid && hist && lane == 0) hist[0] = E;
            continue;
        }
        if (valid && hist && lane == 0) hist[s + 1] = E;
        if (E < best) {
            best = E;
            best_sweep = s + 1;
            if (valid && a.best_state) {
                uint8_t* out = a.best_state + ch * Q;
                for (int c = lane; c < Q; c += GW) out[c] = hts[c];
            }
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
            rung = now;  // the slot keeps its counters: only the rung moves
        }
        if (valid && rhist && lane == 0) rhist[s + 1] = (uint8_t)rung;
    }
    if (!valid) return;
    uint8_t* out = a.state_out + ch * Q;
    for (int c = lane; c < Q; c += GW) out[c] = hts[c];
    if (lane == 0) {
        mcq_post::store_heatbath_figures(a, ch, e_in, E, best, best_sweep, changed);
        if (a.rung_out) a.rung_out[ch] = (uint8_t)rung;
        if (a.n_exchanges) a.n_exchanges[ch] = exchanges;
    }
    if (a.pair_accepted && tl < R - 1) a.pair_accepted[lad * (R - 1) + tl] = accepted;
}

// the padding of a board's lines and the lanes of a chain, as mcq_heatbath_device chooses them; 0 beyond N = 64 (two heights per lane
// there: 96 KB of placements per chain, so that no ladder fits)
int line_padding(int N) { return N <= 8 ? 8 : N <= 12 ? 12 : N <= 16 ? 16 : N <= 24 ? 24 : N <= 32 ? 32 : N <= 64 ? 64 : 128; }
int group_lanes(int N) { return N <= 16 ? 16 : N <= 32 ? 32 : 64; }

// dwords of LDS of one ladder, a multiple of 4 (a second ladder's chain regions stay 16-byte aligned)
long long ladder_words(int N, int R, int D) {
    const long long NP = line_padding(N);
    return (R * (6 * NP * NP / 4) + (long long)R * D + 3 * R + 3) / 4 * 4;
}

// the counter form: the padding of its chain region, and the dwords of LDS of one ladder -- R regions, the staged rows, the event
int counters_padding(int N) { return N <= 8 ? 8 : N <= 12 ? 12 : 16; }
long long counters_ladder_words(int N, int R, int D) {
    return ((long long)R * mcq_columns::counter_region_bytes(counters_padding(N)) + 4ll * R * D + 12 * R) / 4;
}
// the largest workgroup of the counter form, N = 16 with 16 replicas and the longest table, stays within a workgroup's LDS: so does every other
static_assert(16 * mcq_columns::counter_region_bytes(16) + 4 * 16 * MCQ_MAX_HEATBATH_TABLE + 12 * 16 <= MCQ_MAX_TEMPER_LDS, "counter ladder");

long long events_of(long long first, long long n, long long K) { return (first + n) / K - first / K; }

// what both entry points refuse
int check_temper(const mcq_temper* q) {
    if (!q) return fail(g_temper_err, MCQ_EINVAL, "mcq_temper: NULL parameter block");
    if (q->mode != MCQ_MODE_BOARD) return fail(g_temper_err, MCQ_EINVAL, "mode: the tempered heat-bath sweep runs boards only (MCQ_MODE_BOARD), got %d", (int)q->mode);
    if (q->N < MCQ_MIN_N || q->N > MCQ_MAX_N_BOARD) return fail(g_temper_err, MCQ_EINVAL, "N out of range [%d, %d]: %d", MCQ_MIN_N, MCQ_MAX_N_BOARD, (int)q->N);
    if (q->n_chains < 1 || q->n_chains > INT_MAX) return fail(g_temper_err, MCQ_EINVAL, "n_chains out of range [1, 2^31 - 1]: %lld", (long long)q->n_chains);
    const long long R = (long long)q->replicas, K = (long long)q->exchange_every;
    if (R != 2 && R != 4 && R != 8 && R != 16) return fail(g_temper_err, MCQ_EINVAL, "replicas must be 2, 4, 8 or 16, got %lld", R);
    if (q->n_chains % R) return fail(g_temper_err, MCQ_EINVAL, "replicas (%lld) must divide n_chains (%lld)", R, (long long)q->n_chains);
    if (q->n_sweeps < 0) return fail(g_temper_err, MCQ_EINVAL, "n_sweeps must be >= 0, got %lld", (long long)q->n_sweeps);
    if (q->first_sweep < 0) return fail(g_temper_err, MCQ_EINVAL, "first_sweep must be >= 0, got %lld", (long long)q->first_sweep);
    const uint64_t end = (uint64_t)q->first_sweep + (uint64_t)q->n_sweeps, Q = (uint64_t)q->N * (uint64_t)q->N;
    if (end > (uint64_t)INT64_MAX / Q)
        return fail(g_temper_err, MCQ_EINVAL, "first_sweep + n_sweeps = %llu: the word index (first_sweep + n_sweeps) N^2 must stay below 2^63", (unsigned long long)end);
    if (K < 1) return fail(g_temper_err, MCQ_EINVAL, "exchange_every must be >= 1, got %lld", K);
    if (end / (uint64_t)K > (uint64_t)INT64_MAX / (uint64_t)R)
        return fail(g_temper_err, MCQ_EINVAL, "exchange_every = %lld: the word index of the exchange stream, events times replicas, must stay below 2^63", K);
    const long long events = events_of((long long)q->first_sweep, (long long)q->n_sweeps, K);
    if (q->n_events != events)
        return fail(g_temper_err, MCQ_EINVAL, "n_events must be floor((first_sweep + n_sweeps) / exchange_every) - floor(first_sweep / exchange_every) = %lld, got %lld",
                    events, (long long)q->n_events);
    if (q->table_len < 1 || q->table_len > MCQ_MAX_HEATBATH_TABLE)
        return fail(g_temper_err, MCQ_EINVAL, "table_len out of range [1, %d]: %lld", MCQ_MAX_HEATBATH_TABLE, (long long)q->table_len);
    if (q->swap_len < 1 || q->swap_len > MCQ_MAX_TEMPER_SWAP_TABLE)
        return fail(g_temper_err, MCQ_EINVAL, "swap_len out of range [1, %d]: %lld", MCQ_MAX_TEMPER_SWAP_TABLE, (long long)q->swap_len);
    if (!q->seeds) return fail(g_temper_err, MCQ_EINVAL, "seeds is required");
    if (!q->table && q->n_sweeps > 0) return fail(g_temper_err, MCQ_EINVAL, "table is required (n_sweeps x replicas rows of table_len words)");
    if (!q->swap_table && events > 0) return fail(g_temper_err, MCQ_EINVAL, "swap_table is required (n_events x (replicas - 1) rows of swap_len words)");
    if (!q->state_in) return fail(g_temper_err, MCQ_EINVAL, "state_in is required");
    if (!q->state_out) return fail(g_temper_err, MCQ_EINVAL, "state_out is required");
    if ((q->energy_hist || q->rung_hist) && q->hist_stride < q->n_sweeps + 1)
        return fail(g_temper_err, MCQ_EINVAL, "hist_stride must be >= n_sweeps + 1 = %lld, got %lld", (long long)q->n_sweeps + 1, (long long)q->hist_stride);
    return MCQ_OK;
}

// what the host entry point refuses on top of that: it reads the table and the rungs, which the device entry point cannot
int check_temper_inputs(const mcq_temper* q) {
    const long long D = (long long)q->table_len, R = (long long)q->replicas;
    for (long long s = 0; s < q->n_sweeps; s++)
        for (long long t = 0; t < R; t++)
            for (long long d = 0; d < D; d++)
                if (q->table[(s * R + t) * D + d] > (1u << MCQ_HEATBATH_WEIGHT_BITS))
                    return fail(g_temper_err, MCQ_EINVAL, "table: the entry of sweep %lld, rung %lld at index %lld is %u, above 2^%d (W must stay below 2^32)",
                                s, t, d, (unsigned)q->table[(s * R + t) * D + d], MCQ_HEATBATH_WEIGHT_BITS);
    if (q->rung_in)
        for (long long g = 0; g < q->n_chains / R; g++) {
            unsigned seen = 0;
            for (long long r = 0; r < R; r++) {
                const int t = q->rung_in[g * R + r];
                if (t >= R || (seen >> t & 1u))
                    return fail(g_temper_err, MCQ_EINVAL, "rung_in: the rungs of ladder %lld are no permutation of 0 .. %lld (slot %lld holds %d)", g, R - 1, r, t);
                seen |= 1u << t;
            }
        }
    return MCQ_OK;
}

template <int GW, int NP>
hipError_t launch_temper(TemperArgs a, hipStream_t s) {
    const int threads = temper_threads(a.R, GW), lpb = threads / (a.R * GW);
    const size_t bytes = (size_t)lpb * a.ladder_words * 4;
    if (bytes > 32 * 1024) {  // (the default limit is 64 KiB; a ladder takes up to 160)
        const hipError_t e = hipFuncSetAttribute((const void*)mcq_temper_kernel<GW, NP>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((mcq_temper_kernel<GW, NP>), dim3((unsigned)((a.n_ladders + lpb - 1) / lpb)), dim3(threads), bytes, s, a);
    return hipGetLastError();
}

template <int NP, int R>
hipError_t launch_temper_counters(const TemperArgs& a, hipStream_t s) {
    constexpr int threads = temper_threads(R, 16), lpb = threads / (R * 16);
    const size_t bytes = (size_t)lpb * a.ladder_words * 4;
    if (bytes > 32 * 1024) {  // (the default limit is 64 KiB; a ladder takes up to 154 816 bytes)
        const hipError_t e = hipFuncSetAttribute((const void*)mcq_temper_counters_kernel<NP, R>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((mcq_temper_counters_kernel<NP, R>), dim3((unsigned)((a.n_ladders + lpb - 1) / lpb)), dim3(threads), bytes, s, a);
    return hipGetLastError();
}

template <int NP>
hipError_t launch_temper_counters_of(const TemperArgs& a, hipStream_t s) {
    return a.R == 2 ? launch_temper_counters<NP, 2>(a, s) : a.R == 4 ? launch_temper_counters<NP, 4>(a, s)
         : a.R == 8 ? launch_temper_counters<NP, 8>(a, s) : launch_temper_counters<NP, 16>(a, s);
}

// the parameter block as the kernels take it; `words` = the dwords of LDS of one ladder
TemperArgs temper_args(const mcq_temper* q, long long words) {
    return TemperArgs{q->seeds, q->table, q->swap_table, q->rung_in, q->rung_out, q->state_in, q->state_out, q->energy_in, q->energy_out, q->best_energy,
                      q->best_sweep, q->best_state, q->n_changed, q->energy_hist, q->n_exchanges, q->rung_hist, q->pair_accepted, (long long)q->hist_stride,
                      (long long)(q->n_chains / q->replicas), (long long)q->n_sweeps, (long long)q->first_sweep, (long long)q->exchange_every,
                      (long long)(q->first_sweep / q->exchange_every), (int)q->table_len, (int)q->swap_len, (int)q->replicas, (int)words, (int)q->N};
}

// one chain's sweep on the host with the row T: mcq_heatbath_host's, E and n_changed moved
void host_sweep(uint8_t* h, int N, int D, const uint32_t* T, uint64_t w0, uint32_t seed, int* a, uint32_t* C, int& E, long long& changed) {
    const int Q = N * N;
    for (int c = 0; c < Q; c++) {
        host_counts(h, N, c / N, c % N, a);
        int a_min = a[0];
        for (int k = 1; k < N; k++) a_min = a[k] < a_min ? a[k] : a_min;
        uint32_t sum = 0;
        for (int k = 0; k < N; k++) {
            const int d = a[k] - a_min;
            sum += T[d < D - 1 ? d : D - 1];
            C[k] = sum;
        }
        const uint64_t w = w0 + (uint64_t)c;
        uint32_t r[4];
        philox_block((uint32_t)(w >> 2), (uint32_t)(w >> 34), seed, 1u, r);
        const uint32_t U = (uint32_t)(((uint64_t)r[w & 3] * (uint64_t)sum) >> 32);
        int kn = 0;
        while (kn < N - 1 && C[kn] <= U) kn++;  // (a table with T[0] = 0 gives W = 0: the last height, nothing leaves the arrays)
        const int cur = h[c];
        E += a[kn] - a[cur];
        changed += kn != cur;
        h[c] = (uint8_t)kn;
    }
}

}  // namespace

extern "C" {

const char* mcq_temper_last_error(void) { return g_temper_err; }

int mcq_temper_host(const mcq_temper* q) {
    int rc = check_temper(q);
    if (rc == MCQ_OK) rc = check_temper_inputs(q);
    if (rc != MCQ_OK) return rc;
    const int N = q->N, Q = N * N, D = (int)q->table_len, R = (int)q->replicas, DX = (int)q->swap_len;
    const long long K = (long long)q->exchange_every, before = (long long)q->first_sweep / K;
    mcq_post::for_chains(q->n_chains / R, [=](long long first, long long last) {
        std::vector<uint8_t> h((size_t)R * Q);
        std::vector<int> a((size_t)N), E((size_t)R), e_in((size_t)R), best((size_t)R), rung((size_t)R), by_rung((size_t)R);
        std::vector<uint32_t> C((size_t)N);
        std::vector<long long> best_sweep((size_t)R), changed((size_t)R), exchanges((size_t)R), accepted((size_t)R);
        for (long long g = first; g < last; g++) {
            const long long c0 = g * R;
            for (int r = 0; r < R; r++) {
                const long long ch = c0 + r;
                uint8_t* hr = h.data() + (size_t)r * Q;
                const uint8_t* in = q->state_in + ch * Q;
                for (int c = 0; c < Q; c++) hr[c] = (uint8_t)(in[c] < N ? in[c] : N - 1);
                long long twoE = 0;
                for (int c = 0; c < Q; c++) {
                    host_counts(hr, N, c / N, c % N, a.data());
                    twoE += a[hr[c]];
                }
                E[r] = e_in[r] = best[r] = (int)(twoE / 2);
                best_sweep[r] = changed[r] = exchanges[r] = accepted[r] = 0;
                rung[r] = q->rung_in ? q->rung_in[ch] : r;
                if (q->energy_hist) q->energy_hist[ch * q->hist_stride] = E[r];
                if (q->rung_hist) q->rung_hist[ch * q->hist_stride] = (uint8_t)rung[r];
                if (q->best_state)
                    for (int c = 0; c < Q; c++) q->best_state[ch * Q + c] = hr[c];
            }
            const uint32_t seed0 = q->seeds[c0];
            for (long long s = 0; s < q->n_sweeps; s++) {
                const uint64_t w0 = (uint64_t)(q->first_sweep + s) * (uint64_t)Q;
                for (int r = 0; r < R; r++) {
                    const long long ch = c0 + r;
                    uint8_t* hr = h.data() + (size_t)r * Q;
                    host_sweep(hr, N, D, q->table + (s * R + rung[r]) * D, w0, q->seeds[ch], a.data(), C.data(), E[r], changed[r]);
                    if (q->energy_hist) q->energy_hist[ch * q->hist_stride + s + 1] = E[r];
                    if (E[r] < best[r]) {
                        best[r] = E[r];
                        best_sweep[r] = s + 1;
                        if (q->best_state)
                            for (int c = 0; c < Q; c++) q->best_state[ch * Q + c] = hr[c];
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
                uint8_t* out = q->state_out + ch * Q;
                for (int c = 0; c < Q; c++) out[c] = h[(size_t)r * Q + c];
                mcq_post::store_heatbath_figures(*q, ch, e_in[r], E[r], best[r], best_sweep[r], changed[r]);
                if (q->rung_out) q->rung_out[ch] = (uint8_t)rung[r];
                if (q->n_exchanges) q->n_exchanges[ch] = exchanges[r];
                if (q->pair_accepted && r < R - 1) q->pair_accepted[g * (R - 1) + r] = accepted[r];
            }
        }
    });
    return MCQ_OK;
}

int mcq_temper_device(const mcq_temper* q, void* hip_stream) {
    const int rc = check_temper(q);
    if (rc != MCQ_OK) return rc;
    const int N = q->N, R = (int)q->replicas, D = (int)q->table_len;
    const int lpb = temper_threads(R, group_lanes(N)) / (R * group_lanes(N));
    const long long words = ladder_words(N, R, D), bytes = lpb * words * 4;
    if (N > 64 || bytes > MCQ_MAX_TEMPER_LDS)
        return fail(g_temper_err, MCQ_EINVAL, "N = %d with replicas = %d: a ladder takes %lld bytes of LDS, above the %d of a workgroup (mcq_temper_device runs N <= 32 with "
                    "every ladder and N <= 64 with 2 or 4 replicas; mcq_temper_host runs every N)", N, R, bytes, MCQ_MAX_TEMPER_LDS);
    const TemperArgs a = temper_args(q, words);
    hipStream_t s = (hipStream_t)hip_stream;
    hipError_t e;
    if (N <= 8) e = launch_temper<16, 8>(a, s);
    else if (N <= 12) e = launch_temper<16, 12>(a, s);
    else if (N <= 16) e = launch_temper<16, 16>(a, s);
    else if (N <= 24) e = launch_temper<32, 24>(a, s);
    else if (N <= 32) e = launch_temper<32, 32>(a, s);
    else e = launch_temper<64, 64>(a, s);
    if (e != hipSuccess) return fail(g_temper_err, MCQ_EDEVICE, "mcq_temper_device: %s", hipGetErrorString(e));
    return MCQ_OK;
}

int mcq_temper_counters_device(const mcq_temper* q, void* hip_stream) {
    const int rc = check_temper(q);
    if (rc != MCQ_OK) return rc;
    if (q->N > MCQ_MAX_N_TEMPER_COUNTERS)
        return fail(g_temper_err, MCQ_EINVAL, "N = %d: the counter form of the tempered heat-bath sweep runs N <= %d (MCQ_MAX_N_TEMPER_COUNTERS); mcq_temper_device runs "
                    "every N a ladder fits", (int)q->N, MCQ_MAX_N_TEMPER_COUNTERS);
    const int N = q->N;
    const TemperArgs a = temper_args(q, counters_ladder_words(N, (int)q->replicas, (int)q->table_len));
    hipStream_t s = (hipStream_t)hip_stream;
    const hipError_t e = N <= 8 ? launch_temper_counters_of<8>(a, s) : N <= 12 ? launch_temper_counters_of<12>(a, s) : launch_temper_counters_of<16>(a, s);
    if (e != hipSuccess) return fail(g_temper_err, MCQ_EDEVICE, "mcq_temper_counters_device: %s", hipGetErrorString(e));
    return MCQ_OK;
}

}  // extern "C"
