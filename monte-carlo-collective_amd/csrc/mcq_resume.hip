// mcq_resume.hip -- the two kernels that let a chain go on where an earlier call left it (include/mcq.h: mcq_run_device_from,
// mcq_checkpoint_device).  Both sit outside the sweep: mcq_restore_kernel builds the chain records the sweep attaches to from a
// caller's placements and MT19937 states (in the place of mcq_init_kernel), mcq_checkpoint_kernel turns what the sweep left in the
// records back into MT19937 states as np.random.get_state() holds them.  Organised like the init kernel: several chains per
// wavefront, one wavefront per workgroup, no barrier between wavefronts (a __syncthreads() of one wavefront orders LDS phases).
//
// The stream in a record (csrc/mcq_record.h, Stream::attach in csrc/mcq_hip.hip): words [0, ge) of the current generation, words
// [ge, 624) of the one before -- the sweep twists a generation in place, 16 words at a time, as its words are needed.  NumPy holds the
// 624 words of ONE generation and a position.  So the restore kernel REWINDS the words behind the position (rounded up to 64), and the
// checkpoint kernel brings the record to one generation again, the one the read position is in: it finishes the twist forward, or --
// when the sweep has already twisted the first blocks of the next generation while the position is still in the tail of this one --
// rewinds those blocks.
//   twist:  new[i] = x_i ^ (y_i >> 1) ^ (y_i odd ? A : 0),  y_i = (old[i] & UPPER) | (old[i + 1] & LOWER),
//           x_i = old[i + 397] for i < 227, new[i - 227] from there on (and y_623 takes new[0]'s low bits).
//   rewind: A has its top bit set and y_i >> 1 has not, so new[i] ^ x_i gives y_i back; old[j] = (y_j & UPPER) | (y_{j-1} & LOWER).
// Neither direction is a serial walk: for i >= 227 the third input of the rewind is a NumPy word, below it a word >= 397 that the
// first phase has rewound; forward, the words [0, 227), [227, 454) and [454, 624) each depend on the range before only.  The lanes of
// a chain share each phase.  (The low 31 bits of old[0] go into no later word; the sweep keeps them: REC_OLD0.)
//
// Built for gfx950 only, with csrc/mcq_hip.hip:  hipcc --offload-arch=gfx950 -O3 -ffp-contract=off
#include "mcq_record.h"

#include "../../include/mcq.h"

namespace {

constexpr uint32_t MT_UPPER = 0x80000000u, MT_LOWER = 0x7fffffffu, MT_A = 0x9908b0dfu;

// the word the twist makes from old[i] (top bit), old[i + 1] (low 31 bits) and x
__device__ __forceinline__ uint32_t twist_of(uint32_t cur, uint32_t nxt, uint32_t x) {
    const uint32_t y = (cur & MT_UPPER) | (nxt & MT_LOWER);
    return x ^ (y >> 1) ^ ((y & 1u) ? MT_A : 0u);
}
// y_i from new[i] ^ x_i
__device__ __forceinline__ uint32_t untwist_y(uint32_t t) {
    const uint32_t odd = t >> 31;
    if (odd) t ^= MT_A;
    return (t << 1) | odd;
}
// every byte of w clamped to at most m
__device__ __forceinline__ uint32_t clamp_bytes(uint32_t w, uint32_t m) {
    uint32_t r = 0;
#pragma unroll
    for (int b = 0; b < 4; b++) r |= min((w >> (8 * b)) & 0xffu, m) << (8 * b);
    return r;
}

// ------------------------------------------------------------------------------------------------
// restore kernel: CI chains per wavefront, L = 64 / CI lanes each.
// LDS per chain (lds_words): mt[624] | y[624] (the rewind's scratch), later: state bytes | one family of E0 line counters
// A state that is no placement cannot make the sweep leave its tables: every coordinate is clamped to N - 1 here (two queens of a
// full_3d state on one cell share a column bit, which miscounts energies and touches nothing else); a position above 624 reads as 624.
// ------------------------------------------------------------------------------------------------
template <int CI>
__global__ __launch_bounds__(64) void mcq_restore_kernel(McqRestoreArgs a, int lds_words) {
    extern __shared__ uint32_t lds[];
    constexpr int L = 64 / CI;
    const int lane = threadIdx.x, sub = lane & (L - 1), grp = lane / L;
    const long long mine = (long long)blockIdx.x * CI + grp;
    const bool valid = mine < a.n_chains;
    const long long chain = valid ? mine : a.n_chains - 1;  // (an idle group repeats the last chain in its own LDS slice and writes nothing)
    const int N = a.N, Q = a.Q;
    uint32_t* mt = lds + (size_t)grp * lds_words;
    uint32_t* y = mt + MT_N;
    uint32_t* rec = a.ws + chain * (long long)a.rec_words;

    // ---- stream ----
    int rpos = 0, ge = 0;  // NumPy's position 624, and a fresh seed: the first draw starts a generation
    if (a.stream) {
        const uint32_t* g = a.stream + chain * 625LL;
        for (int p = sub; p < MT_N; p += L) mt[p] = g[p];
        const uint32_t np = g[MT_N];
        if (np < (uint32_t)MT_N) rpos = (int)np, ge = (rpos + 63) & ~63, ge = ge > MT_N ? MT_N : ge;
        __syncthreads();
        // phase 1: y_i for i >= 227 from NumPy's words alone, then the words from 228 on; phase 2: the rest, with rewound third inputs.
        // (bounds per chain, every lane walks every phase: the chains of a wavefront stand at different positions)
        const bool rew = np < (uint32_t)MT_N && ge < MT_N;  // (position 624: the key IS the generation before the one the next draw starts)
        const int y1 = rew ? (ge - 1 > 227 ? ge - 1 : 227) : MT_N, w1 = rew ? (ge > 228 ? ge : 228) : MT_N;
        for (int i = y1 + sub; i < MT_N; i += L) y[i] = untwist_y(mt[i] ^ mt[i - 227]);
        __syncthreads();
        for (int j = w1 + sub; j < MT_N; j += L) mt[j] = (y[j] & MT_UPPER) | (y[j - 1] & MT_LOWER);
        __syncthreads();
        const int y2 = rew && ge <= 227 ? (ge > 0 ? ge - 1 : 0) : 227, w2 = rew && ge <= 227 ? ge : 228;
        for (int i = y2 + sub; i < 227; i += L) y[i] = untwist_y(mt[i] ^ mt[i + MT_M]);
        __syncthreads();
        for (int j = w2 + sub; j < 228; j += L) mt[j] = (y[j] & MT_UPPER) | ((j > 0 ? y[j - 1] : mt[0]) & MT_LOWER);  // (old[0]: only its upper bit is ever read)
        __syncthreads();
    } else {  // init_genrand: key[p] = s; s = 1812433253 * (s ^ (s >> 30)) + p + 1 (np.random.seed), nothing drawn
        uint32_t s = a.seeds[chain];
        for (int p = 0; p < MT_N; p++) {
            if (sub == (p & (L - 1))) mt[p] = s;
            s = 1812433253u * (s ^ (s >> 30)) + (uint32_t)p + 1u;
        }
        __syncthreads();
    }
    if (valid) {
        for (int w = sub; w < MT_N / 4; w += L) ((uint4*)rec)[w] = ((const uint4*)mt)[w];  // (records are 64-byte aligned)
        if (sub == 0) rec[REC_MIRROR] = mt[0], rec[REC_POS] = (uint32_t)rpos, rec[REC_GEN_END] = (uint32_t)ge;
    }
    __syncthreads();  // the state takes the place of y

    // ---- state ----
    uint8_t* st = (uint8_t*)(mt + MT_N);
    const int st_words = (a.state_bytes + 3) / 4;
    uint32_t* cnt = (uint32_t*)st + st_words;
    const uint32_t top = (uint32_t)(N - 1);
    const uint8_t* src = a.state + chain * (long long)a.state_bytes;
    if ((a.state_bytes & 15) == 0) {  // rows of a 16-byte aligned array stay aligned
        for (int w = sub; w < a.state_bytes / 16; w += L) {
            uint4 v = ((const uint4*)src)[w];
            v.x = clamp_bytes(v.x, top), v.y = clamp_bytes(v.y, top), v.z = clamp_bytes(v.z, top), v.w = clamp_bytes(v.w, top);
            ((uint4*)st)[w] = v;
        }
    } else {
        for (int c = sub; c < a.state_bytes; c += L) st[c] = (uint8_t)min((uint32_t)src[c], top);
    }
    __syncthreads();
    int e = mcq_count_e0(st, cnt, N, Q, a.mode == MCQ_MODE_BOARD, sub, L);
    for (int o = 1; o < L; o <<= 1) e += __shfl_xor(e, o, 64);

    if (!valid) return;
    if (sub == 0) {
        rec[REC_E0] = (uint32_t)e;
        if (a.initial_energy) a.initial_energy[chain] = e;
        if (a.stream_words) a.stream_words[chain] = 0u;  // the sweep adds its own
    }
    if ((a.state_bytes & 15) == 0) {  // REC_STATE is a 16-byte multiple into a 64-byte aligned record
        uint4* rst = (uint4*)(rec + REC_STATE);
        for (int w = sub; w < a.state_bytes / 16; w += L) rst[w] = ((const uint4*)st)[w];
    } else {
        uint8_t* rst = (uint8_t*)(rec + REC_STATE);
        for (int c = sub; c < a.state_bytes; c += L) rst[c] = st[c];
    }
    if (a.mode == MCQ_MODE_FULL3D && a.qtab) {
        if (N > 32) {
            uint32_t* qt = (uint32_t*)a.qtab + chain * (long long)a.qtab_stride;
            for (int c = sub; c < Q; c += L) qt[c] = (uint32_t)st[3 * c] | ((uint32_t)st[3 * c + 1] << 8) | ((uint32_t)st[3 * c + 2] << 16);
        } else {
            uint16_t* qt = a.qtab + chain * (long long)a.qtab_stride;
            for (int c = sub; c < Q; c += L) qt[c] = (uint16_t)(st[3 * c] | (st[3 * c + 1] << 5) | (st[3 * c + 2] << 10));
        }
    }
}

// ------------------------------------------------------------------------------------------------
// checkpoint kernel: four chains per wavefront, 16 lanes each.  LDS per chain: W[624] (the record's words) | O[624] (the state to write).
// The record says where the sweep stopped twisting (csrc/mcq_record.h: REC_BOUNDARY = gen, REC_GEN_END = pos, counts of words;
// gi = gen mod 624, ahead = gen - pos): nothing is inferred from the words.
//   gi == 0                 all 624 words are one generation; position 624 - ahead
//   gi > 0, ahead <  gi     the position (gi - ahead >= 1) is in the generation of words [0, gi): twist [gi, 624) forward
//   gi > 0, ahead >= gi     the position (624 + gi - ahead) is still in the generation before: rewind [0, gi), word 0 from REC_OLD0
// The result is what NumPy itself holds after as many draws: one generation, position 1 .. 624.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void mcq_checkpoint_kernel(const uint32_t* __restrict__ ws, int rec_words, long long n_chains, uint32_t* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[4 * 2 * MT_N];
    constexpr int L = 16;
    const int lane = threadIdx.x, sub = lane & (L - 1), grp = lane / L;
    const long long mine = (long long)blockIdx.x * 4 + grp;
    const bool valid = mine < n_chains;
    const long long chain = valid ? mine : n_chains - 1;
    uint32_t* W = lds + grp * 2 * MT_N;
    uint32_t* O = W + MT_N;
    const uint32_t* rec = ws + chain * (long long)rec_words;
    for (int w = sub; w < MT_N / 4; w += L) {
        const uint4 v = ((const uint4*)rec)[w];
        ((uint4*)W)[w] = v, ((uint4*)O)[w] = v;
    }
    const uint32_t gen = rec[REC_BOUNDARY], old0 = rec[REC_OLD0];
    const int gi = (int)(gen % (uint32_t)MT_N) & ~15;  // (a multiple of 16 below 624)
    int ahead = (int)(gen - rec[REC_GEN_END]);
    ahead = ahead < 0 ? 0 : ahead > 64 ? 64 : ahead;  // (what a sweep writes is inside these bounds)
    const bool fwd = gi > 0 && ahead < gi, rew = gi > 0 && ahead >= gi;
    const int pos = gi == 0 ? MT_N - ahead : fwd ? gi - ahead : MT_N + gi - ahead;
    __syncthreads();
    // forward: [gi, 227) from old words, [227, 454) and [454, 624) from the range before (bounds per chain, every lane walks every phase)
    const int a0 = fwd ? gi : MT_N, b0 = fwd ? (gi > 227 ? gi : 227) : MT_N, c0 = fwd ? (gi > 454 ? gi : 454) : MT_N;
    for (int i = a0 + sub; i < 227; i += L) O[i] = twist_of(W[i], W[i + 1], W[i + MT_M]);
    __syncthreads();
    for (int i = b0 + sub; i < 454; i += L) O[i] = twist_of(W[i], W[i + 1], O[i - 227]);
    __syncthreads();
    for (int i = c0 + sub; i < MT_N; i += L) O[i] = twist_of(W[i], W[i + 1 == MT_N ? 0 : i + 1], O[i - 227]);  // (word 0 is of the new generation: gi > 0)
    __syncthreads();
    // rewind of [0, gi), gi <= 64: the third inputs, words 397 .., have not been twisted yet
    const int r1 = rew ? gi : 0;
    uint32_t yv[4];
#pragma unroll
    for (int t = 0; t < 4; t++) {
        const int i = sub + t * L;
        yv[t] = i < r1 ? untwist_y(W[i] ^ W[i + MT_M]) : 0u;
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < 4; t++) {
        const int i = sub + t * L;
        if (i < r1) W[i] = yv[t];
    }
    __syncthreads();
    for (int j = sub; j < r1; j += L) O[j] = j == 0 ? old0 : (W[j] & MT_UPPER) | (W[j - 1] & MT_LOWER);
    __syncthreads();
    if (!valid) return;
    uint32_t* row = out + chain * 625LL;  // (rows of 625 words: 4-byte aligned only)
    for (int p = sub; p < MT_N; p += L) row[p] = O[p];
    if (sub == 0) row[MT_N] = (uint32_t)pos;
}

size_t restore_lds_words(const McqRestoreArgs& a) {
    const size_t D = 2 * (size_t)a.N - 1, cnt_words = (D * D + 3) / 4, st_words = ((size_t)a.state_bytes + 3) / 4;
    const size_t behind = st_words + cnt_words > (size_t)MT_N ? st_words + cnt_words : (size_t)MT_N;
    return ((size_t)MT_N + behind + 3) & ~(size_t)3;
}

}  // namespace

hipError_t mcq_launch_restore(const McqRestoreArgs& a, hipStream_t s) {
    const size_t words = restore_lds_words(a), bytes1 = words * 4;
    if (bytes1 > 160 * 1024) return hipErrorInvalidValue;
    // as many chains per wavefront as leave a CU 8 wavefronts (the init kernel's rule)
    const int ci = 4 * bytes1 * 8 <= 160 * 1024 ? 4 : 2 * bytes1 * 8 <= 160 * 1024 ? 2 : 1;
    const size_t bytes = ci * bytes1;
    const unsigned grid = (unsigned)((a.n_chains + ci - 1) / ci);
    hipError_t e;
    if (ci == 4) {
        e = hipFuncSetAttribute((const void*)mcq_restore_kernel<4>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if (e == hipSuccess) hipLaunchKernelGGL(mcq_restore_kernel<4>, dim3(grid), dim3(64), bytes, s, a, (int)words);
    } else if (ci == 2) {
        e = hipFuncSetAttribute((const void*)mcq_restore_kernel<2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if (e == hipSuccess) hipLaunchKernelGGL(mcq_restore_kernel<2>, dim3(grid), dim3(64), bytes, s, a, (int)words);
    } else {
        e = hipFuncSetAttribute((const void*)mcq_restore_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if (e == hipSuccess) hipLaunchKernelGGL(mcq_restore_kernel<1>, dim3(grid), dim3(64), bytes, s, a, (int)words);
    }
    return e == hipSuccess ? hipGetLastError() : e;
}

hipError_t mcq_launch_checkpoint(const uint32_t* ws, int rec_words, long long n_chains, uint32_t* stream_out, hipStream_t s) {
    hipLaunchKernelGGL(mcq_checkpoint_kernel, dim3((unsigned)((n_chains + 3) / 4)), dim3(64), 0, s, ws, rec_words, n_chains, stream_out);
    return hipGetLastError();
}
