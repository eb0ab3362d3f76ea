// mcq_columns.h -- the lane helpers of the board heat-bath column update, shared by csrc/mcq_heatbath.hip and csrc/mcq_temper.hip: the
// lanes of a GROUP (16, 32 or 64 of a wavefront) are the candidate heights of one column.  DPP row rotations and shifts for the
// minimum and the prefix sum over a group, and the test of one line of LDS cells against a lane's heights.  Moved here as they stood
// in mcq_heatbath.hip; the device code of that file's kernels is what it was (profiles/tempering_refactor.md).  The layout of the counter
// form's chain region (counter_offset and its two sizes) stands here for the same reason: both counter kernels read it from one place
// (profiles/tempering_counters.md).
#ifndef MCQ_COLUMNS_H
#define MCQ_COLUMNS_H

#include <hip/hip_runtime.h>

#include <cstdint>

namespace mcq_columns {

// DPP within a row of 16 lanes: the value of the lane `n` below (0 where the row ends) / of the lane n to the right, cyclically
template <int n>
__device__ __forceinline__ uint32_t row_shr(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x110 + n, 0xF, 0xF, false);
}
template <int n>
__device__ __forceinline__ int row_ror(int v) {
    return __builtin_amdgcn_update_dpp(v, v, 0x120 + n, 0xF, 0xF, false);
}

template <int GW>
__device__ __forceinline__ int group_min(int v) {
    v = min(v, row_ror<1>(v));
    v = min(v, row_ror<2>(v));
    v = min(v, row_ror<4>(v));
    v = min(v, row_ror<8>(v));
    for (int o = 16; o < GW; o <<= 1) v = min(v, __shfl_xor(v, o, GW));
    return v;
}

// inclusive prefix sum over the lanes of a group; `total` = the group's sum
template <int GW>
__device__ __forceinline__ uint32_t group_scan(uint32_t v, int lane, uint32_t& total) {
    v += row_shr<1>(v);
    v += row_shr<2>(v);
    v += row_shr<4>(v);
    v += row_shr<8>(v);
    if (GW == 16) {
        total = __shfl(v, 15, GW);
        return v;
    }
    const uint32_t r0 = __shfl(v, 15, GW), r1 = __shfl(v, 31, GW);
    uint32_t add = lane >= 16 ? r0 : 0;
    total = r0 + r1;
    if (GW == 64) {
        const uint32_t r2 = __shfl(v, 47, GW), r3 = __shfl(v, 63, GW);
        add += (lane >= 32 ? r1 : 0) + (lane >= 48 ? r2 : 0);
        total += r2 + r3;
    }
    return v + add;
}

// the cells of one line (NP bytes, 255 = no cell) against this lane's heights: a cell at index idx of height hp counts when
// |hp - k| is 0 or |idx - pos|
template <int KPL, int NP>
__device__ __forceinline__ void line_hits(const uint32_t* line, int pos, int k0, int k1, int& c0, int& c1) {
    constexpr int UN = NP <= 32 ? NP / 4 : 4;
#pragma unroll UN
    for (int w = 0; w < NP / 4; w++) {
        const uint32_t v = line[w];
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const int hp = (int)((v >> (8 * b)) & 255u);
            const int d = abs(4 * w + b - pos);
            const int a0 = abs(hp - k0);
            c0 += (a0 == 0) | (a0 == d);
            if (KPL == 2) {
                const int a1 = abs(hp - k1);
                c1 += (a1 == 0) | (a1 == d);
            }
        }
    }
}

// ---- the counter form (N <= 16): where a chain keeps the queen counts of the cube's 12 line families, one byte per line ----
// A counter is at
//   line (5N - 2) + v,   line = i | N + j | 3N - 1 + i - j | 4N - 1 + i + j   (6N - 2 lines in the plane),
//                        v = k | 2N - 1 - pos + k | 3N - 1 + pos + k          (height step 0, +1, -1; pos = j along a row, i otherwise),
// so the lanes of a group, the heights k, read 16 consecutive bytes per family.  counter_offset is the address at k = 0.
__device__ __forceinline__ int counter_offset(int dir, int step, int i, int j, int N) {
    const int line = dir == 0 ? i : dir == 1 ? N + j : dir == 2 ? 3 * N - 1 + i - j : 4 * N - 1 + i + j;
    const int pos = dir == 0 ? j : i;
    const int v = step == 0 ? 0 : step == 1 ? 2 * N - 1 - pos : 3 * N - 1 + pos;
    return line * (5 * N - 2) + v;
}

// bytes of a chain's counters at the padding NP (8, 12 or 16: a multiple of 4), and of its whole region -- the counters and ONE copy of
// the heights, 64 bytes off a multiple of 128, so that the two chains of a half-wavefront read different banks: 1 856, 4 288, 7 616
__host__ __device__ constexpr int counter_bytes(int NP) { return (6 * NP - 2) * (5 * NP - 2); }
__host__ __device__ constexpr int counter_region_bytes(int NP) { return (counter_bytes(NP) + NP * NP + 63) / 128 * 128 + 64; }

}  // namespace mcq_columns

#endif
