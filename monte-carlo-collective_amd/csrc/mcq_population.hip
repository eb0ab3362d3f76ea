// mcq_population.hip -- population annealing: the kernels that resample the chains of a population between two segments
// (include/mcq.h: mcq_resample).  They sit outside the sweep like the restore / checkpoint kernels of csrc/mcq_resume.hip: a
// finished segment leaves final_energy and final_state in device memory, the plan kernel picks a parent for every slot, the rows
// kernel gathers the parents' placements into a second buffer the next segment is restored from, and the fold kernel keeps the
// per-slot summary of the whole run.  Nothing goes to the host.
//
//   plan   in two launches.  scan: one workgroup per population, up to 16 wavefronts.  min-reduce of the energies; then the
//          population in tiles of one element per lane: weight = table[min(E - Emin, D - 1)], inclusive 64-bit scan inside the
//          wavefront with __shfl_up, the wavefront totals through LDS and scanned once more by every wavefront, the tile's total
//          carried in a register.  The prefix sums C_r go to global scratch (a population of 65 536 chains has 512 KiB of them).
//          search: one lane per slot over the whole device -- with both halves in the one workgroup of a 65 536-chain
//          population the 17 dependent loads of each of its 64 bisections per lane were 0.44 ms of a 1.0 ms boundary
//          (profiles/population_annealing.md).  Slot m finds the smallest r with C_r R > m W + U.  C_{R-1} R = W R >
//          (R - 1) W + U, so the search always ends inside the population -- also for a table that is all zero (W = 0: every
//          slot takes r = R - 1).
//   rows   state_out[m] = state_in[parent[m]], and run_best_state[m] = seg_best_state[m] where the segment's best is strictly
//          lower.  16 bytes per lane where the rows are 16-byte multiples, 4 or 1 otherwise.
//   fold   one lane per slot: energy_out[m] = energies[parent[m]] and the scalar half of the summary.  It runs behind the rows
//          kernel, which still compares against the run's old best energy.
//
// Built for gfx950 only, with csrc/mcq_hip.hip:  hipcc --offload-arch=gfx950 -O3 -ffp-contract=off
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdarg>
#include <cstdio>
#include <vector>

#include "../../include/mcq.h"

namespace {

thread_local char g_pop_err[256] = "";

int pop_fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_pop_err, sizeof g_pop_err, fmt, ap);
    va_end(ap);
    return code;
}

constexpr int PLAN_MAX_THREADS = 1024;

// U = floor(x W / 2^32) from the full product: x W = x Whi 2^32 + x Wlo, and both partial products fit 64 bits (W < 2^43)
__host__ __device__ inline unsigned long long pop_offset(uint32_t x, unsigned long long W) {
    return (unsigned long long)x * (W >> 32) + (((unsigned long long)x * (W & 0xffffffffull)) >> 32);
}

__host__ __device__ inline uint32_t pop_weight(const uint32_t* table, int D, int e, int emin) {
    const long long d = (long long)e - (long long)emin;
    return table[d < (long long)(D - 1) ? (int)d : D - 1];
}

struct PlanArgs {
    const int32_t* energies;
    const uint32_t* table;
    const uint32_t* offsets;
    unsigned long long* C;  // scratch, [n_chains]
    int32_t* parent;
    int64_t* stats;
    int R, D;
};

// ---- plan, first half: one workgroup per population.  Leaves C_r in scratch and W, E_min (and a zeroed count) in stats. ----
__global__ __launch_bounds__(PLAN_MAX_THREADS) void mcq_population_scan_kernel(PlanArgs a) {
    __shared__ unsigned long long wave_sum[16];
    __shared__ int wave_min[16];
    const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wave = tid >> 6, nw = nt >> 6;
    const int R = a.R, D = a.D;
    const long long base = (long long)blockIdx.x * R;
    const int32_t* E = a.energies + base;
    unsigned long long* C = a.C + base;

    int mn = INT_MAX;
    for (int r = tid; r < R; r += nt) mn = min(mn, E[r]);
    for (int o = 32; o; o >>= 1) mn = min(mn, __shfl_xor(mn, o, 64));
    if (lane == 0) wave_min[wave] = mn;
    __syncthreads();
    mn = lane < nw ? wave_min[lane] : INT_MAX;
    for (int o = 8; o; o >>= 1) mn = min(mn, __shfl_xor(mn, o, 64));
    mn = __shfl(mn, 0, 64);

    unsigned long long carry = 0;
    for (int t0 = 0; t0 < R; t0 += nt) {
        const int r = t0 + tid;
        unsigned long long v = r < R ? (unsigned long long)pop_weight(a.table, D, E[r], mn) : 0ull;
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned long long u = __shfl_up(v, o, 64);
            if (lane >= o) v += u;
        }
        if (lane == 63) wave_sum[wave] = v;
        __syncthreads();
        unsigned long long s = lane < nw ? wave_sum[lane] : 0ull;  // every wavefront scans the (at most 16) totals for itself
        for (int o = 1; o < 16; o <<= 1) {
            const unsigned long long u = __shfl_up(s, o, 64);
            if (lane >= o) s += u;
        }
        const unsigned long long before = wave ? __shfl(s, wave - 1, 64) : 0ull, total = __shfl(s, nw - 1, 64);
        if (r < R) C[r] = carry + before + v;
        carry += total;
        __syncthreads();  // wave_sum is rewritten by the next tile
    }
    if (tid == 0) {
        int64_t* st = a.stats + 3ll * blockIdx.x;
        st[0] = 0, st[1] = (int64_t)carry, st[2] = (int64_t)mn;
    }
}

// ---- plan, second half: one lane per slot, the whole device.  Bisection over the population's C_r; counts the first children. ----
__global__ __launch_bounds__(256) void mcq_population_search_kernel(PlanArgs a, long long n_chains) {
    const long long slot = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool valid = slot < n_chains;
    const long long s = valid ? slot : n_chains - 1;
    const int R = a.R;
    const long long g = s / R;
    const int m = (int)(s - g * R);
    const unsigned long long* C = a.C + g * R;
    const unsigned long long W = (unsigned long long)a.stats[3 * g + 1], U = pop_offset(a.offsets[g], W), RR = (unsigned long long)R;
    const unsigned long long key = (unsigned long long)m * W + U;
    int lo = 0, hi = R - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (C[mid] * RR > key) hi = mid;
        else lo = mid + 1;
    }
    // the map is monotone: slot m is the first child of its parent iff slot m - 1 has an earlier one, i.e. iff chain lo - 1 passes its test
    const bool first_child = valid && (m == 0 || (lo > 0 && C[lo - 1] * RR > key - W));
    if (valid) a.parent[slot] = (int32_t)(g * R + lo);
    unsigned long long* count = (unsigned long long*)(a.stats + 3 * g);
    if (__all(g == __shfl(g, 0, 64))) {  // the usual case, a wavefront inside one population: one atomic for its 64 slots
        const unsigned long long firsts = __ballot(first_child);
        if ((threadIdx.x & 63) == 0 && firsts) atomicAdd(count, (unsigned long long)__popcll(firsts));
    } else if (first_child) {
        atomicAdd(count, 1ull);
    }
}

struct RowsArgs {
    const void* state_in;
    void* state_out;
    const int32_t* parent;
    const void* seg_best_state;
    void* run_best_state;
    const int32_t* seg_best_energy;
    const int32_t* run_best_energy;
    long long n_chains;
    int vecs;   // vectors of sizeof(V) bytes per row
    int first;  // the first segment: its best state is the run's
};

template <typename V>
__global__ __launch_bounds__(256) void mcq_population_rows_kernel(RowsArgs a) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= a.n_chains * a.vecs) return;
    const long long m = idx / a.vecs;
    const int j = (int)(idx - m * a.vecs);
    if (a.state_in) {
        long long p = a.parent[m];
        p = p < 0 ? 0 : p >= a.n_chains ? a.n_chains - 1 : p;  // (what the plan kernel writes is inside these bounds)
        ((V*)a.state_out)[idx] = ((const V*)a.state_in)[p * a.vecs + j];
    }
    if (a.run_best_state && (a.first || a.seg_best_energy[m] < a.run_best_energy[m])) ((V*)a.run_best_state)[idx] = ((const V*)a.seg_best_state)[idx];
}

struct FoldArgs {
    const int32_t* parent;
    const int32_t* energies;
    int32_t* energy_out;
    const int32_t* seg_best_energy;
    const int64_t* seg_steps_to_best;
    const int64_t* seg_n_accepted;
    const int64_t* seg_near_ties;
    const uint32_t* seg_stream_words;
    int32_t* run_best_energy;
    int64_t* run_steps_to_best;
    int64_t* run_n_accepted;
    int64_t* run_near_ties;
    uint32_t* run_stream_words;
    long long n_chains, first_step;
};

__global__ __launch_bounds__(256) void mcq_population_fold_kernel(FoldArgs a) {
    const long long m = (long long)blockIdx.x * 256 + threadIdx.x;
    if (m >= a.n_chains) return;
    if (a.energy_out) {
        long long p = a.parent[m];
        p = p < 0 ? 0 : p >= a.n_chains ? a.n_chains - 1 : p;
        a.energy_out[m] = a.energies[p];
    }
    if (!a.run_best_energy) return;
    const bool first = a.first_step == 0;
    const int32_t sb = a.seg_best_energy[m];
    if (first || sb < a.run_best_energy[m]) {  // strictly: the first index of the minimum stays where it is on a tie
        a.run_best_energy[m] = sb;
        a.run_steps_to_best[m] = a.first_step + a.seg_steps_to_best[m];
    }
    a.run_n_accepted[m] = (first ? 0 : a.run_n_accepted[m]) + a.seg_n_accepted[m];
    if (a.run_near_ties) a.run_near_ties[m] = (first ? 0 : a.run_near_ties[m]) + a.seg_near_ties[m];
    if (a.run_stream_words) a.run_stream_words[m] = (first ? 0u : a.run_stream_words[m]) + a.seg_stream_words[m];
}

// what both entry points refuse about the plan
int check_plan(const mcq_resample* r) {
    if (!r) return pop_fail(MCQ_EINVAL, "mcq_resample: NULL parameter block");
    if (r->population <= 0 || r->population % 16 || r->population > MCQ_MAX_POPULATION)
        return pop_fail(MCQ_EINVAL, "population must be a positive multiple of 16 and at most %d, got %lld", MCQ_MAX_POPULATION, (long long)r->population);
    if (r->n_chains <= 0 || r->n_chains >= (1ll << 31) || r->n_chains % r->population)
        return pop_fail(MCQ_EINVAL, "n_chains (%lld) must be a positive multiple of the population (%lld) below 2^31", (long long)r->n_chains, (long long)r->population);
    if (r->table_len < 1 || r->table_len > MCQ_MAX_RESAMPLE_TABLE)
        return pop_fail(MCQ_EINVAL, "table_len must be in [1, %d], got %lld", MCQ_MAX_RESAMPLE_TABLE, (long long)r->table_len);
    if (!r->table || !r->offsets || !r->energies || !r->parent || !r->stats)
        return pop_fail(MCQ_EINVAL, "mcq_resample: table, offsets, energies, parent and stats are required");
    return MCQ_OK;
}

bool fold_on(const mcq_resample* r) { return r->run_best_energy != nullptr; }

int check_device(const mcq_resample* r) {
    if (!r) return pop_fail(MCQ_EINVAL, "mcq_resample: NULL parameter block");
    if (r->state_in) {
        const int rc = check_plan(r);
        if (rc != MCQ_OK) return rc;
        if (!r->state_out || r->state_out == r->state_in) return pop_fail(MCQ_EINVAL, "the gather cannot run in place: state_out must be a second buffer");
        if (r->energy_out && r->energy_out == r->energies) return pop_fail(MCQ_EINVAL, "energy_out must not be the energies array");
    } else if (r->n_chains <= 0 || r->n_chains >= (1ll << 31)) {
        return pop_fail(MCQ_EINVAL, "n_chains out of range");
    }
    if (r->state_bytes <= 0 || r->state_bytes > (1ll << 24)) return pop_fail(MCQ_EINVAL, "state_bytes out of range");
    if (!r->state_in && !fold_on(r)) return pop_fail(MCQ_EINVAL, "mcq_resample: neither a state to resample nor a summary to fold");
    if (fold_on(r)) {
        if (r->first_step < 0) return pop_fail(MCQ_EINVAL, "first_step must be >= 0");
        if (!r->seg_best_energy || !r->seg_steps_to_best || !r->seg_n_accepted || !r->run_steps_to_best || !r->run_n_accepted)
            return pop_fail(MCQ_EINVAL, "the summary fold needs best_energy, steps_to_best and n_accepted of the segment and of the run");
        if ((r->run_near_ties != nullptr) != (r->seg_near_ties != nullptr) || (r->run_stream_words != nullptr) != (r->seg_stream_words != nullptr) ||
            (r->run_best_state != nullptr) != (r->seg_best_state != nullptr))
            return pop_fail(MCQ_EINVAL, "near_ties, stream_words and best_state are folded when both the segment's and the run's array are given");
    }
    const uintptr_t align = r->state_bytes % 16 == 0 ? 15 : r->state_bytes % 4 == 0 ? 3 : 0;
    const void* rows[] = {r->state_in, r->state_out, fold_on(r) ? r->seg_best_state : nullptr, fold_on(r) ? r->run_best_state : nullptr};
    for (const void* p : rows)
        if (p && ((uintptr_t)p & align)) return pop_fail(MCQ_EINVAL, "rows of %lld bytes are moved %d bytes at a time: the arrays must be aligned to that", (long long)r->state_bytes, (int)align + 1);
    return MCQ_OK;
}

template <typename V>
void launch_rows(const RowsArgs& a, hipStream_t s) {
    const long long total = a.n_chains * a.vecs;
    hipLaunchKernelGGL(mcq_population_rows_kernel<V>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, a);
}

}  // namespace

extern "C" {

const char* mcq_population_last_error(void) { return g_pop_err; }

size_t mcq_resample_scratch_bytes(const mcq_resample* r) {
    if (!r || r->n_chains <= 0 || r->n_chains >= (1ll << 31)) {
        pop_fail(MCQ_EINVAL, "n_chains out of range");
        return 0;
    }
    return (size_t)r->n_chains * sizeof(unsigned long long);
}

int mcq_resample_plan_host(const mcq_resample* r) {
    const int rc = check_plan(r);
    if (rc != MCQ_OK) return rc;
    const long long R = r->population, pops = r->n_chains / R;
    const int D = (int)r->table_len;
    std::vector<unsigned long long> C((size_t)R);
    for (long long g = 0; g < pops; g++) {
        const int32_t* E = r->energies + g * R;
        int mn = INT_MAX;
        for (long long i = 0; i < R; i++) mn = E[i] < mn ? E[i] : mn;
        unsigned long long W = 0;
        for (long long i = 0; i < R; i++) C[(size_t)i] = (W += pop_weight(r->table, D, E[i], mn));
        const unsigned long long U = pop_offset(r->offsets[g], W);
        long long p = 0, distinct = 0, last = -1;
        for (long long m = 0; m < R; m++) {
            const unsigned long long key = (unsigned long long)m * W + U;
            while (p < R - 1 && !(C[(size_t)p] * (unsigned long long)R > key)) p++;  // (monotone: the search goes on where slot m - 1 ended)
            r->parent[g * R + m] = (int32_t)(g * R + p);
            distinct += p != last;
            last = p;
        }
        r->stats[3 * g] = distinct, r->stats[3 * g + 1] = (int64_t)W, r->stats[3 * g + 2] = mn;
    }
    return MCQ_OK;
}

int mcq_resample_device(const mcq_resample* r, void* scratch, size_t scratch_bytes, void* hip_stream) {
    const int rc = check_device(r);
    if (rc != MCQ_OK) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    const bool fold = fold_on(r);
    if (r->state_in) {
        if (!scratch || ((uintptr_t)scratch & 7) || scratch_bytes < mcq_resample_scratch_bytes(r))
            return pop_fail(MCQ_ENOMEM, "mcq_resample_device: scratch of %zu bytes, 8-byte aligned, needed", mcq_resample_scratch_bytes(r));
        PlanArgs pa{r->energies, r->table, r->offsets, (unsigned long long*)scratch, r->parent, r->stats, (int)r->population, (int)r->table_len};
        const int threads = r->population >= PLAN_MAX_THREADS ? PLAN_MAX_THREADS : (int)((r->population + 63) / 64) * 64;
        hipLaunchKernelGGL(mcq_population_scan_kernel, dim3((unsigned)(r->n_chains / r->population)), dim3(threads), 0, s, pa);
        hipLaunchKernelGGL(mcq_population_search_kernel, dim3((unsigned)((r->n_chains + 255) / 256)), dim3(256), 0, s, pa, (long long)r->n_chains);
    }
    const bool fold_state = fold && r->run_best_state;
    if (r->state_in || fold_state) {
        RowsArgs ra{r->state_in, r->state_out, r->parent, fold_state ? r->seg_best_state : nullptr, fold_state ? r->run_best_state : nullptr,
                    r->seg_best_energy, r->run_best_energy, (long long)r->n_chains, 0, r->first_step == 0};
        if (r->state_bytes % 16 == 0) ra.vecs = (int)(r->state_bytes / 16), launch_rows<uint4>(ra, s);
        else if (r->state_bytes % 4 == 0) ra.vecs = (int)(r->state_bytes / 4), launch_rows<uint32_t>(ra, s);
        else ra.vecs = (int)r->state_bytes, launch_rows<uint8_t>(ra, s);
    }
    const bool gather_e = r->state_in && r->energy_out;
    if (gather_e || fold) {
        FoldArgs fa{r->parent, r->energies, gather_e ? r->energy_out : nullptr, r->seg_best_energy, r->seg_steps_to_best, r->seg_n_accepted,
                    r->seg_near_ties, r->seg_stream_words, fold ? r->run_best_energy : nullptr, r->run_steps_to_best, r->run_n_accepted,
                    r->run_near_ties, r->run_stream_words, (long long)r->n_chains, (long long)r->first_step};
        hipLaunchKernelGGL(mcq_population_fold_kernel, dim3((unsigned)((r->n_chains + 255) / 256)), dim3(256), 0, s, fa);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return pop_fail(MCQ_EDEVICE, "mcq_resample_device: %s", hipGetErrorString(e));
    return MCQ_OK;
}

}  // extern "C"
