// mcq_columns.h -- the lane helpers of the board heat-bath column update, shared by csrc/mcq_heatbath.hip and csrc/mcq_temper.hip: the
// lanes of a GROUP (16, 32 or 64 of a wavefront) are the candidate heights of one column.  DPP row rotations and shifts for the
// minimum and the prefix sum over a group, and the test of one line of LDS cells against a lane's heights.  Moved here as they stood
// in mcq_heatbath.hip; the device code of that file's kernels is what it was (profiles/tempering_refactor.md).
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

}  // namespace mcq_columns

#endif
