// mcq_record.h -- what csrc/mcq_hip.hip (init + sweep) and csrc/mcq_resume.hip (restore + checkpoint) share: the layout of a chain
// record in the workspace, the E0 count, and the launchers of the two resume kernels.
#ifndef MCQ_RECORD_H
#define MCQ_RECORD_H

#include <hip/hip_runtime.h>

#include <cstdint>

constexpr int MT_N = 624;
constexpr int MT_M = 397;
constexpr int REC_MIRROR = 624;   // record word: copy of MT word 0, so that words i+1 and i+397.. of a block never wrap inside a lane's run
constexpr int REC_POS = 625;      // record word: MT index of the next word to consume
constexpr int REC_GEN_END = 626;  // record word: words [0, gen_end) belong to the current generation
constexpr int REC_E0 = 627;       // record word: initial energy
constexpr int REC_STATE = 628;    // first word of the state bytes (heights or (i,j,k) triplets)
// What the sweep LEAVES in a record (mcq_checkpoint_kernel reads it; nothing else does):
//   REC_GEN_END  pos: the stream's read position as a count of words -- it started at REC_POS (mcq_stream_words_kernel subtracts the two)
//   REC_MIRROR   REC_BOUNDARY: gen, the count of twisted words on the same scale (it started at the record's gen_end, so gen mod 624 is the
//                MT index the twist stopped at): words [0, gen mod 624) of the record belong to the generation the sweep twisted last, the
//                rest to the one before, and gen - pos (0..64) twisted words have not been consumed.  Written by the sweep's epilogue, when
//                the mirror has no reader left.  (32-bit counts: a segment that is to be checkpointed stays below 2^32 words.)
//   REC_E0       REC_OLD0: word 0 of the generation BEFORE the one whose block 0 the sweep twisted last (written with that block, E0 having
//                been read in the prologue).  The low 31 bits of a generation's word 0 go into no later word, so they cannot be
//                rewound from anything else.
// Both stores go through the address of a store the sweep made anyway, with an instruction offset: a separate address is a 64-bit value the
// compiler keeps in two vector registers across the step loop (measured: +2 VGPRs in 88 of the 133 sweep instantiations).
constexpr int REC_BOUNDARY = REC_MIRROR;
constexpr int REC_OLD0 = REC_E0;

// E0 = number of unordered attacking pairs (mcmc_board.py:82-122, mcmc.py:134-169).  Two distinct cells attack iff they
// share one of the 13 lines through a cell, and no two cells share more than one, so E0 = sum over lines of c (c - 1) / 2
// with c the queens on the line: one byte counter per line (c <= N), O(Q) increments instead of Q^2 / 2 pair tests.
//   N^2 lines each:        (j, k) along i | (i, k) along j | (i, j) along k
//   N (2N - 1) lines each: (k, i - j), (k, i + j) | (j, i - k), (j, i + k) | (i, j - k), (i, j + k)      planar diagonals
//   (2N - 1)^2 lines each: (i - j, i - k), (i - j, i + k), (i + j, i - k), (i + j, i + k)                space diagonals
// One family at a time in a (2N - 1)^2-byte array `cnt` of the chain's LDS slice: all 13 at once are 30 N^2 bytes, which keeps a CU to
// few chains at N = 12 and does not fit at all beyond N = 70.  `st` is the chain's state in LDS; the L lanes of the chain (sub = 0 .. L - 1)
// share the work and each returns its part of the sum.  Every lane of the workgroup (one wavefront) must call it.
__device__ __forceinline__ int mcq_count_e0(const uint8_t* st, uint32_t* cnt, int N, int Q, bool board, int sub, int L) {
    int e = 0;
    const int D = 2 * N - 1, o = N - 1;
    for (int f = 0; f < 13; f++) {
        if (f == 2 && board) continue;  // lines along k: on a board the column (i, j) itself, one queen each
        const int lines = f < 3 ? N * N : f < 9 ? N * D : D * D;
        for (int w = sub; w < (lines + 3) / 4; w += L) cnt[w] = 0;
        __syncthreads();  // (a workgroup of one wavefront: orders the phases for the compiler as well)
        for (int c = sub; c < Q; c += L) {
            int i, j, k;
            if (board) i = c / N, j = c % N, k = st[c];
            else i = st[3 * c], j = st[3 * c + 1], k = st[3 * c + 2];
            int line;
            switch (f) {
            case 0: line = j * N + k; break;
            case 1: line = i * N + k; break;
            case 2: line = i * N + j; break;
            case 3: line = k * D + (i - j + o); break;
            case 4: line = k * D + (i + j); break;
            case 5: line = j * D + (i - k + o); break;
            case 6: line = j * D + (i + k); break;
            case 7: line = i * D + (j - k + o); break;
            case 8: line = i * D + (j + k); break;
            case 9: line = (i - j + o) * D + (i - k + o); break;
            case 10: line = (i - j + o) * D + (i + k); break;
            case 11: line = (i + j) * D + (i - k + o); break;
            default: line = (i + j) * D + (i + k); break;
            }
            atomicAdd(&cnt[line >> 2], 1u << (8 * (line & 3)));
        }
        __syncthreads();
        for (int w = sub; w < (lines + 3) / 4; w += L) {
            const uint32_t x = cnt[w];
#pragma unroll
            for (int b = 0; b < 4; b++) {
                const int c = (int)((x >> (8 * b)) & 0xffu);
                e += c * (c - 1) / 2;
            }
        }
        __syncthreads();
    }
    return e;
}

// mcq_restore_kernel (csrc/mcq_resume.hip): chain records from the caller's placements and MT19937 states, in the place of the init kernel.
struct McqRestoreArgs {
    int N, Q, mode;
    int state_bytes, rec_words;
    long long n_chains;
    uint32_t* ws;            // chain records
    const uint8_t* state;    // [n_chains][state_bytes]
    const uint32_t* stream;  // [n_chains][625] as np.random.get_state() holds them, or NULL: seed from seeds[r]
    const uint32_t* seeds;
    uint16_t* qtab;          // full_3d: the packed queen table of the workspace (uint32 entries beyond N = 32), or NULL
    int qtab_stride;
    int32_t* initial_energy;  // optional
    uint32_t* stream_words;   // optional: 0 (a restored chain takes no initialisation draws)
};
hipError_t mcq_launch_restore(const McqRestoreArgs& a, hipStream_t s);
// mcq_checkpoint_kernel: the records a sweep left behind -> MT19937 states as NumPy holds them, uint32[n_chains][625]
hipError_t mcq_launch_checkpoint(const uint32_t* ws, int rec_words, long long n_chains, uint32_t* stream_out, hipStream_t s);

#endif  // MCQ_RECORD_H
