// mcq_field.h -- the ATTACK FIELD of a full_3d placement, which csrc/mcq_quench3d.hip and csrc/mcq_heatbath3d.hip both live on: its device
// form in LDS, its host form, and the launch of a kernel that uses it.  S(t) = the number of queens that hold or attack cell t, one entry
// per cell.  With queen q at p taken out (S -= 1 on p and on the in-bounds cells of the 13 lines through p), S(t) IS a(q, t) for every t.
//
//   layout  one chain per workgroup of W lanes (64, 256 or 1024: one, four or sixteen wavefronts), behind the kernel's own dwords:
//             field   one byte per cell while 13 (N - 1) + 1 <= 255 (N <= 19), 16 bits beyond (64 KiB at N = 32), read as whole dwords
//             occ     the occupancy bitmap, N^3 bits; the pad bits behind the last cell are set, so no scan tests cell < N^3
//             queens  Q packed cells i << 10 | j << 5 | k, 16 bits each (132 KiB with everything at N = 32, Q = N^3 - 1)
//   update  The lines through p meet only in p, so one queen's update touches distinct cells, but two cells share a dword: the update
//           is a 32-bit LDS atomic add of +-1 << the cell's bit offset.  A byte never carries: it holds at most 13 (N - 1) + 1, and
//           the cell a queen is taken from counted that queen.  A lane's slot of an update is (direction, signed step), STEPS = 32
//           or 64 steps per direction, so the slot decodes with shifts.
//   repeat  A REPEATED placement (two queens in one cell after clamping) breaks the byte bound and is never put into the field: its
//           counts come from a pairwise scan, Q^2 / W tests per lane, and it is written back unmoved.
//   barrier Nothing here but block_min and block_sum holds a barrier: the barriers between these steps stay in the kernels, where the
//           branches around them can be seen to be uniform over the workgroup.
//   host    HostField: the same field with an int per cell, a byte per cell for the occupancy and plain loops.
#ifndef MCQ_FIELD_H
#define MCQ_FIELD_H

#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

namespace mcq_field {

// direction d = 0 .. 12: the half of {-1, 0, 1}^3 \ {0} whose first non-zero component is +1, as the digits of d + 14 in base 3
__host__ __device__ __forceinline__ void direction(int d, int& di, int& dj, int& dk) {
    const int c = d + 14;
    di = c / 9 - 1, dj = (c / 3) % 3 - 1, dk = c % 3 - 1;
}

// the non-zero ones among |di|, |dj|, |dk| are all equal (the same cell included: a shared cell counts as an attacking pair)
__host__ __device__ __forceinline__ bool attacks(int pa, int pb) {
    const int di = abs((pa >> 10) - (pb >> 10)), dj = abs(((pa >> 5) & 31) - ((pb >> 5) & 31)), dk = abs((pa & 31) - (pb & 31));
    const int m = max(di, max(dj, dk));
    return (di == 0 || di == m) && (dj == 0 || dj == m) && (dk == 0 || dk == m);
}

// a packed cell i << 10 | j << 5 | k  <->  its index (i N + j) N + k
__device__ __forceinline__ int cell_of(int p, int N) { return ((p >> 10) * N + ((p >> 5) & 31)) * N + (p & 31); }
__device__ __forceinline__ int packed_of(int cell, int N, int N2) {
    const int i = cell / N2, j = (cell - i * N2) / N;
    return i << 10 | j << 5 | (cell - i * N2 - j * N);
}

// BARRIER: whether a barrier stands in front of the exchange through red (the readers of the reduction before this one are done with
// red).  The quench needs it.  The heat bath has none: between the readers of one queen's minimum and the writers of the next lie the
// barriers of the update.
template <int W, bool BARRIER>
__device__ __forceinline__ uint32_t block_min(uint32_t v, uint32_t* red) {
    for (int o = 32; o; o >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, o, 64));
    if (W == 64) return v;
    if (BARRIER) __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    v = red[0];
    for (int w = 1; w < W / 64; w++) v = min(v, red[w]);
    return v;
}

template <int W>
__device__ __forceinline__ int block_sum(int v, uint32_t* red) {
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o, 64);
    if (W == 64) return v;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = (uint32_t)v;
    __syncthreads();
    v = (int)red[0];
    for (int w = 1; w < W / 64; w++) v += (int)red[w];
    return v;
}

// S(cell) of a field of BITS-wide entries
template <int BITS>
__device__ __forceinline__ int field_at(const uint32_t* field, int cell) {
    constexpr int CPD = 32 / BITS;  // cells per dword
    return (int)((field[cell / CPD] >> ((cell % CPD) * BITS)) & ((1u << BITS) - 1u));
}

// S += sign on the cell p (packed) and on every in-bounds cell of the 13 lines through it: this lane's slots of queen p
template <int W, int BITS, int STEPS>
__device__ __forceinline__ void put(uint32_t* field, int N, int p, int sign, int first_slot, int stride, int n_slots) {
    constexpr int CPD = 32 / BITS;
    const int pi = p >> 10, pj = (p >> 5) & 31, pk = p & 31;
    for (int s = first_slot; s < n_slots; s += stride) {
        const int d = s / STEPS, step = (s % STEPS) - (N - 1);  // step = -(N - 1) .. N - 1 where s % STEPS <= 2 N - 2
        int di, dj, dk;
        direction(d, di, dj, dk);
        const int i = pi + step * di, j = pj + step * dj, k = pk + step * dk;
        const bool on = step < N && (step != 0 || d == 0) && (unsigned)i < (unsigned)N && (unsigned)j < (unsigned)N && (unsigned)k < (unsigned)N;
        if (on) {
            const int cell = (i * N + j) * N + k;
            const uint32_t one = 1u << ((cell % CPD) * BITS);
            atomicAdd(&field[cell / CPD], sign > 0 ? one : 0u - one);
        }
    }
}

// a chain's field, occupancy and queens in LDS: fw dwords of field, bw dwords of occ (adjacent), then the queens
struct Chain {
    uint32_t* field;
    uint32_t* occ;
    uint16_t* queens;
    int fw, bw;
};

// the layout behind `base` for C = N^3 cells
template <int BITS>
__device__ __forceinline__ Chain carve(uint32_t* base, int C) {
    constexpr int CPD = 32 / BITS;
    const int fw = (C + CPD - 1) / CPD, bw = (C + 31) / 32;
    uint32_t* occ = base + fw;
    return Chain{base, occ, (uint16_t*)(occ + bw), fw, bw};
}

// The start of a chain is three steps with a barrier behind each: the clear of field and occ; the pad bits, by ONE lane; the clamped
// load, queen by queen.  (The helpers below hold no loop: a helper with a loop of its own is optimised apart from its kernel and changed
// the kernels' code; the loops over queens, slots and words are the kernels'.)
__device__ __forceinline__ void set_pad_bits(uint32_t* occ, int bw, int C) {
    if (C & 31) occ[bw - 1] = ~0u << (C & 31);  // the pad bits: never a candidate
}

// queen q from the chain's bytes, clamped to N - 1, into queens and occ; true where the cell was taken already (a repeated placement)
__device__ __forceinline__ int load_queen(uint16_t* queens, uint32_t* occ, const uint8_t* in, int N, int q) {
    const int i = min((int)in[3 * q], N - 1), j = min((int)in[3 * q + 1], N - 1), k = min((int)in[3 * q + 2], N - 1);
    queens[q] = (uint16_t)(i << 10 | j << 5 | k);
    const int cell = (i * N + j) * N + k;
    const uint32_t bit = 1u << (cell & 31);
    return (atomicOr(&occ[cell >> 5], bit) & bit) != 0;
}

// the field of all queens is every (queen, slot) pair x = 0 .. Q 13 STEPS - 1, one atomic add each
template <int W, int BITS, int STEPS>
__device__ __forceinline__ void put_slot(uint32_t* field, const uint16_t* queens, int N, int x) {
    constexpr int SLOTS = 13 * STEPS;
    put<W, BITS, STEPS>(field, N, queens[x / SLOTS], +1, x % SLOTS, SLOTS, SLOTS);
}

// the queens that attack the queen at p (packed), which the field counts: 2 E is the sum of this over the queens
template <int BITS>
__device__ __forceinline__ int attackers_at(const uint32_t* field, int N, int p) {
    return field_at<BITS>(field, cell_of(p, N)) - 1;
}

__device__ __forceinline__ void store_queen(uint8_t* out, int q, int p) {
    out[3 * q] = (uint8_t)(p >> 10), out[3 * q + 1] = (uint8_t)((p >> 5) & 31), out[3 * q + 2] = (uint8_t)(p & 31);
}

__device__ __forceinline__ void store_queens(uint8_t* out, const uint16_t* queens, int Q, int tid, int W) {
    for (int q = tid; q < Q; q += W) store_queen(out, q, queens[q]);
}

// what ONE lane does next to put(.., -1) when a queen leaves `cell`, and next to put(.., +1) when queen q enters t = cell tcell
__device__ __forceinline__ void vacate(uint32_t* occ, int cell) { occ[cell >> 5] &= ~(1u << (cell & 31)); }
__device__ __forceinline__ void occupy(uint32_t* occ, uint16_t* queens, int q, int t, int tcell) {
    occ[tcell >> 5] |= 1u << (tcell & 31);
    queens[q] = (uint16_t)t;
}

// ---- launch ----
// the instantiation table: lanes per chain, field width, steps per direction of an update (2 N - 1 <= STEPS)
template <int W_, int BITS_, int STEPS_>
struct Shape {
    static constexpr int W = W_, BITS = BITS_, STEPS = STEPS_;
};

template <class F>
hipError_t for_shape_of(int N, F&& f) {
    if (N <= 12) return f(Shape<64, 8, 32>{});
    if (N <= 19) return f(Shape<256, 8, 64>{});
    return f(Shape<1024, 16, 64>{});
}

// one chain per workgroup of S::W lanes, with `extra` dwords of dynamic LDS in front of the field
template <class S, class Args>
hipError_t launch(void (*kernel)(Args), const Args& a, int N, int Q, int extra, long long n_chains, hipStream_t s) {
    const int cells = N * N * N, cpd = 32 / S::BITS;
    const size_t bytes = 4 * (size_t)(extra + (cells + cpd - 1) / cpd + (cells + 31) / 32 + (Q + 1) / 2);
    if (bytes > 32 * 1024) {  // (the default limit is 64 KiB with the kernel's static LDS; a chain at N = 32 takes up to 132 KiB and its extra)
        const hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kernel, dim3((unsigned)n_chains), dim3(S::W), bytes, s, a);
    return hipGetLastError();
}

// ---- host ----
// the field with an int per cell; cells are indices (i N + j) N + k here, pos[n] = the cell of queen n
struct HostField {
    int N, Q, N2, C;
    std::vector<int> S, pos;
    std::vector<uint8_t> occ;

    HostField(int N_, int Q_) : N(N_), Q(Q_), N2(N_ * N_), C(N_ * N_ * N_), S((size_t)C), pos((size_t)Q_), occ((size_t)C) {}

    // S += sign on the cell and on the 13 lines through it
    void put(int cell, int sign) {
        const int pi = cell / N2, pj = (cell / N) % N, pk = cell % N;
        S[(size_t)cell] += sign;
        for (int d = 0; d < 13; d++) {
            int di, dj, dk;
            direction(d, di, dj, dk);
            for (int step = -(N - 1); step < N; step++) {
                const int i = pi + step * di, j = pj + step * dj, k = pk + step * dk;
                if (step != 0 && i >= 0 && i < N && j >= 0 && j < N && k >= 0 && k < N) S[(size_t)((i * N + j) * N + k)] += sign;
            }
        }
    }

    // the field of a chain's bytes, clamped to N - 1; true for a repeated placement (which the host field holds all the same)
    bool load(const uint8_t* in) {
        for (int c = 0; c < C; c++) S[(size_t)c] = 0, occ[(size_t)c] = 0;
        bool repeated = false;
        for (int n = 0; n < Q; n++) {
            const int i = in[3 * n] < N ? in[3 * n] : N - 1, j = in[3 * n + 1] < N ? in[3 * n + 1] : N - 1, k = in[3 * n + 2] < N ? in[3 * n + 2] : N - 1;
            const int cell = (i * N + j) * N + k;
            pos[(size_t)n] = cell;
            repeated |= occ[(size_t)cell] != 0;
            occ[(size_t)cell] = 1;
            put(cell, +1);
        }
        return repeated;
    }

    int energy() const {
        long long twoE = 0;
        for (int n = 0; n < Q; n++) twoE += S[(size_t)pos[(size_t)n]] - 1;
        return (int)(twoE / 2);
    }

    // queen n leaves its cell / enters cell t
    void take_out(int n) {
        put(pos[(size_t)n], -1);
        occ[(size_t)pos[(size_t)n]] = 0;
    }
    void put_back(int n, int t) {
        put(t, +1);
        occ[(size_t)t] = 1;
        pos[(size_t)n] = t;
    }

    void store(uint8_t* out) const {
        for (int n = 0; n < Q; n++) {
            const int p = pos[(size_t)n];
            out[3 * n] = (uint8_t)(p / N2), out[3 * n + 1] = (uint8_t)((p / N) % N), out[3 * n + 2] = (uint8_t)(p % N);
        }
    }
};

}  // namespace mcq_field

#endif
