// nfold3d_host_check.cpp -- a stand-alone program around mcq_nfold3d_host for a sanitizer run of the HOST code of csrc/mcq_nfold3d.hip
// on a CPU: the smallest cube, one in the middle and the largest, few queens, N^2 and a cube with one free cell, inputs with bytes >= N,
// rows from every weight at its bound to a row that forbids every rise, both clocks and a clock of zeros, a run cut in two with the need
// and the event counter carried, every optional output present and every one absent, in place, no segment at all, a repeated placement
// and a refusal.  The host code works through raw pointers into its list of free cells, the caller's rows and history, in blocks of 512
// differences; this run is what guards them.  No GPU is touched.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -o nfold3d_host_check \
//         tools/nfold3d_host_check.cpp monte-carlo-collective_amd/csrc/mcq_nfold3d.hip && ./nfold3d_host_check
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../include/mcq.h"

namespace {

int failures = 0;

void expect(bool ok, const char* what, int N, int Q) {
    if (!ok) {
        std::printf("FAILED: %s at N = %d, Q = %d (%s)\n", what, N, Q, mcq_nfold3d_last_error());
        failures++;
    }
}

std::vector<uint32_t> rows(const std::vector<double>& betas, int D) {
    std::vector<uint32_t> t(betas.size() * (size_t)D);
    for (size_t s = 0; s < betas.size(); s++)
        for (int d = 0; d < D; d++) t[s * (size_t)D + (size_t)d] = (uint32_t)std::floor(16777216.0 * std::exp(-betas[s] * d));
    return t;
}

struct Buffers {
    std::vector<uint8_t> out, best;
    std::vector<int32_t> e_in, e_out, e_best, hist, flags;
    std::vector<int64_t> step, events, up, flat;
    std::vector<uint64_t> need, weight;
    Buffers(int n, int Q, int S)
        : out((size_t)(3 * n * Q)), best((size_t)(3 * n * Q)), e_in((size_t)n), e_out((size_t)n), e_best((size_t)n), hist((size_t)(n * (S + 1))), flags((size_t)n),
          step((size_t)n), events((size_t)n), up((size_t)n), flat((size_t)n), need((size_t)n), weight((size_t)n) {}
    void point(mcq_nfold3d& q, int S) {
        q.state_out = out.data(), q.best_state = best.data(), q.energy_in = e_in.data(), q.energy_out = e_out.data(), q.best_energy = e_best.data();
        q.best_step = step.data(), q.events_out = events.data(), q.n_uphill = up.data(), q.n_flat = flat.data(), q.need_out = need.data();
        q.weight_out = weight.data(), q.energy_hist = hist.data(), q.hist_stride = S + 1, q.flags = flags.data();
    }
};

// n placements of Q distinct cells, cell (7 r + 11 n) mod N^3 onwards with a stride coprime to N^3; some bytes that equal N - 1 are raised
std::vector<uint8_t> placements(int N, int Q, int n) {
    const int C = N * N * N, stride = C % 5 ? 5 : 7;
    std::vector<uint8_t> s((size_t)(3 * n * Q));
    for (int r = 0; r < n; r++)
        for (int i = 0; i < Q; i++) {
            const int cell = (int)(((long long)i * stride + 7 * r) % C);
            uint8_t* p = &s[(size_t)(3 * (r * Q + i))];
            p[0] = (uint8_t)(cell / (N * N)), p[1] = (uint8_t)((cell / N) % N), p[2] = (uint8_t)(cell % N);
            for (int k = 0; k < 3; k++)
                if (p[k] == N - 1 && (i + k) % 3 == 0) p[k] = (uint8_t)(N + 40 + k);
        }
    return s;
}

void run(int N, int Q, int n, int steps) {
    const int S = 4, D = 64;
    const std::vector<uint32_t> t = rows({0.0, 0.7, 2.0, 30.0}, D);
    const std::vector<uint8_t> in = placements(N, Q, n);
    std::vector<uint32_t> seeds((size_t)n), exp_clock(256), mean_clock(256, 1u << 24), zero_clock(256, 0u);
    for (int r = 0; r < n; r++) seeds[(size_t)r] = 4000000000u + (uint32_t)r;
    for (int i = 0; i < 256; i++) exp_clock[(size_t)i] = (uint32_t)std::llround(-16777216.0 * std::log((256.0 + i + 0.5) / 512.0));
    mcq_nfold3d q;
    std::memset(&q, 0, sizeof q);
    q.N = N, q.mode = MCQ_MODE_FULL3D, q.n_queens = Q, q.n_chains = n, q.n_segs = S, q.seg_steps = steps;
    q.seeds = seeds.data(), q.table = t.data(), q.table_len = D, q.state_in = in.data();
    q.clock_table = exp_clock.data(), q.clock_ln2 = 11629080;
    Buffers whole(n, Q, S), a(n, Q, 2), b(n, Q, 2), slim(n, Q, S);
    whole.point(q, S);
    expect(mcq_nfold3d_host(&q) == MCQ_OK, "the whole run", N, Q);
    // the run cut in two, the need and the event counter carried
    mcq_nfold3d first = q, second = q;
    first.n_segs = 2, a.point(first, 2);
    expect(mcq_nfold3d_host(&first) == MCQ_OK, "the first piece", N, Q);
    second.n_segs = 2, second.first_seg = 2, second.table = t.data() + 2 * D, second.state_in = a.out.data(), second.need_in = a.need.data(), second.events_in = a.events.data();
    b.point(second, 2);
    expect(mcq_nfold3d_host(&second) == MCQ_OK, "the second piece", N, Q);
    expect(b.out == whole.out && b.e_out == whole.e_out && b.events == whole.events && b.need == whole.need && b.weight == whole.weight, "the cut run is the unbroken run", N, Q);
    // no optional output, in place
    mcq_nfold3d bare = q;
    slim.out = in;
    bare.state_in = bare.state_out = slim.out.data();
    bare.best_state = nullptr, bare.energy_in = bare.energy_out = bare.best_energy = nullptr, bare.best_step = bare.events_out = bare.n_uphill = bare.n_flat = nullptr;
    bare.need_out = bare.weight_out = nullptr, bare.energy_hist = nullptr, bare.flags = nullptr;
    expect(mcq_nfold3d_host(&bare) == MCQ_OK && slim.out == whole.out, "no optional output, in place", N, Q);
    // the other clocks; a clock of zeros over one step of one segment
    mcq_nfold3d mean = q;
    mean.clock_table = mean_clock.data(), mean.clock_ln2 = 0;
    expect(mcq_nfold3d_host(&mean) == MCQ_OK, "the mean clock", N, Q);
    if ((long long)Q * (N * N * N - Q) < 4000) {
        mcq_nfold3d zero = q;
        zero.clock_table = zero_clock.data(), zero.clock_ln2 = 0, zero.n_segs = 1, zero.seg_steps = 1;
        expect(mcq_nfold3d_host(&zero) == MCQ_OK && whole.events[0] == 4096, "a clock of zeros fires 4096 events", N, Q);
    }
    // no segment at all; a repeated placement; a refusal
    mcq_nfold3d none = q;
    none.n_segs = 0, none.table = nullptr;
    expect(mcq_nfold3d_host(&none) == MCQ_OK && whole.weight[0] == 0, "no segment", N, Q);
    std::vector<uint8_t> rep = in;
    rep[3] = rep[0], rep[4] = rep[1], rep[5] = rep[2];
    mcq_nfold3d twice = q;
    twice.state_in = rep.data();
    expect(mcq_nfold3d_host(&twice) == MCQ_OK && whole.flags[0] == MCQ_NFOLD3D_REPEATED && whole.weight[0] == 0, "a repeated placement", N, Q);
    mcq_nfold3d bad = q;
    bad.n_queens = N * N * N;
    expect(mcq_nfold3d_host(&bad) == MCQ_EINVAL, "Q = N^3 is refused", N, Q);
}

}  // namespace

int main() {
    run(2, 2, 3, 5), run(2, 7, 3, 5), run(3, 9, 4, 6), run(5, 124, 3, 4), run(13, 169, 3, 3), run(13, 600, 2, 2), run(32, 5, 2, 3), run(32, 1024, 1, 1);
    std::printf(failures ? "%d check(s) FAILED\n" : "nfold3d_host_check: every check passed\n", failures);
    return failures != 0;
}
