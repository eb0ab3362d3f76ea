// nfold_host_check.cpp -- a stand-alone program around mcq_nfold_host for a sanitizer run of the HOST code of csrc/mcq_nfold.hip on a
// CPU: the smallest board, one in the middle and the largest, inputs with bytes >= N, rows from every weight at its bound to a row
// that forbids every rise, both clocks and a clock of zeros, a run cut in two with the need and the event counter carried, every
// optional output present and every one absent, in place, no segment at all, and a refusal.  The host code works through pointers into
// its own table of ints, the caller's rows and history; this run is what guards them.  No GPU is touched.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -o nfold_host_check \
//         tools/nfold_host_check.cpp monte-carlo-collective_amd/csrc/mcq_nfold.hip && ./nfold_host_check
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../include/mcq.h"

namespace {

int failures = 0;

void expect(bool ok, const char* what, int N) {
    if (!ok) {
        std::printf("FAILED: %s at N = %d (%s)\n", what, N, mcq_nfold_last_error());
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
    std::vector<int32_t> e_in, e_out, e_best, hist;
    std::vector<int64_t> step, events, up, flat;
    std::vector<uint64_t> need, weight;
    Buffers(int n, int Q, int S)
        : out((size_t)(n * Q)), best((size_t)(n * Q)), e_in((size_t)n), e_out((size_t)n), e_best((size_t)n), hist((size_t)(n * (S + 1))), step((size_t)n),
          events((size_t)n), up((size_t)n), flat((size_t)n), need((size_t)n), weight((size_t)n) {}
    void point(mcq_nfold& q, int S) {
        q.state_out = out.data(), q.best_state = best.data();
        q.energy_in = e_in.data(), q.energy_out = e_out.data(), q.best_energy = e_best.data();
        q.best_step = step.data(), q.events_out = events.data(), q.n_uphill = up.data(), q.n_flat = flat.data();
        q.need_out = need.data(), q.weight_out = weight.data(), q.energy_hist = hist.data(), q.hist_stride = S + 1;
    }
};

void run(int N, int n, int steps) {
    const int Q = N * N, D = MCQ_MAX_NFOLD_TABLE, S = 4;
    std::vector<uint8_t> in((size_t)(n * Q));
    uint32_t x = 12345u + (uint32_t)N;
    for (auto& b : in) {
        x = x * 1664525u + 1013904223u;
        b = (uint8_t)((x >> 8) % (uint32_t)(N + 3));  // some bytes >= N: clamped
    }
    std::vector<uint32_t> seeds((size_t)n);
    for (int r = 0; r < n; r++) seeds[(size_t)r] = 4294967290u + (uint32_t)r;  // wraps past 2^32
    const std::vector<uint32_t> tab = rows({0.0, 0.7, 2.0, 40.0}, D);  // the last row: T[d > 0] = 0
    std::vector<uint32_t> expclk(256), meanclk(256, 1u << 24), zeroclk(256, 0u);
    for (int i = 0; i < 256; i++) expclk[(size_t)i] = (uint32_t)std::llround(-16777216.0 * std::log((256.0 + i + 0.5) / 512.0));
    const int64_t ln2 = std::llround(16777216.0 * std::log(2.0));

    mcq_nfold q{};
    q.N = N, q.mode = MCQ_MODE_BOARD, q.n_chains = n, q.n_segs = S, q.first_seg = 0, q.seg_steps = steps;
    q.seeds = seeds.data(), q.table = tab.data(), q.table_len = D, q.clock_table = expclk.data(), q.clock_ln2 = ln2, q.state_in = in.data();
    Buffers whole(n, Q, S);
    whole.point(q, S);
    expect(mcq_nfold_host(&q) == MCQ_OK, "the whole run", N);

    // cut in two: the second piece takes the first's placements, need and event counter
    Buffers a(n, Q, S), b(n, Q, S);
    mcq_nfold qa = q, qb = q;
    qa.n_segs = 1;
    a.point(qa, S);
    expect(mcq_nfold_host(&qa) == MCQ_OK, "the first piece", N);
    qb.n_segs = S - 1, qb.first_seg = 1, qb.table = tab.data() + D, qb.state_in = a.out.data(), qb.need_in = a.need.data(), qb.events_in = a.events.data();
    b.point(qb, S);
    expect(mcq_nfold_host(&qb) == MCQ_OK, "the second piece", N);
    expect(b.out == whole.out && b.events == whole.events && b.need == whole.need && b.e_out == whole.e_out && b.weight == whole.weight, "the cut run is the whole run", N);

    // no optional output, in place
    std::vector<uint8_t> inplace = in;
    mcq_nfold bare{};
    bare.N = N, bare.mode = MCQ_MODE_BOARD, bare.n_chains = n, bare.n_segs = S, bare.seg_steps = steps;
    bare.seeds = seeds.data(), bare.table = tab.data(), bare.table_len = D, bare.clock_table = expclk.data(), bare.clock_ln2 = ln2;
    bare.state_in = inplace.data(), bare.state_out = inplace.data();
    expect(mcq_nfold_host(&bare) == MCQ_OK && inplace == whole.out, "in place, no optional output", N);

    // the mean clock, a clock of zeros over one step, the shortest table, no segment
    Buffers m(n, Q, S);
    mcq_nfold qm = q;
    qm.clock_table = meanclk.data(), qm.clock_ln2 = 0;
    m.point(qm, S);
    expect(mcq_nfold_host(&qm) == MCQ_OK, "the mean clock", N);
    mcq_nfold qz = q;
    qz.clock_table = zeroclk.data(), qz.clock_ln2 = 0, qz.n_segs = 1, qz.seg_steps = 1;
    m.point(qz, S);
    expect(mcq_nfold_host(&qz) == MCQ_OK && m.events[0] == (1 << MCQ_NFOLD_TIME_BITS), "a clock of zeros fires 4096 events in a step", N);
    const uint32_t one[1] = {1u << 24};
    mcq_nfold q1 = q;
    q1.table = one, q1.table_len = 1, q1.n_segs = 1;
    m.point(q1, S);
    expect(mcq_nfold_host(&q1) == MCQ_OK && m.weight[0] == ((uint64_t)Q * (uint64_t)(N - 1) << 24), "a table of one entry", N);
    mcq_nfold q0 = q;
    q0.n_segs = 0, q0.table = nullptr;
    m.point(q0, S);
    expect(mcq_nfold_host(&q0) == MCQ_OK && m.e_in == m.e_out && m.weight[0] == 0, "no segment: a recount and a copy", N);

    // refusals
    mcq_nfold bad = q;
    bad.table_len = MCQ_MAX_NFOLD_TABLE + 1;
    expect(mcq_nfold_host(&bad) == MCQ_EINVAL, "table_len above its bound is refused", N);
    bad = q, bad.hist_stride = S;
    expect(mcq_nfold_host(&bad) == MCQ_EINVAL, "a short history row is refused", N);
}

}  // namespace

int main() {
    run(2, 3, 20);
    run(13, 70, 10);  // more than 64 chains: the host entry's threads
    run(32, 2, 6);
    expect(mcq_nfold_host(nullptr) == MCQ_EINVAL, "a NULL block is refused", 0);
    std::printf(failures ? "%d failures\n" : "nfold_host_check: ok\n", failures);
    return failures ? 1 : 0;
}
