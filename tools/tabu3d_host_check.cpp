// tabu3d_host_check.cpp -- a stand-alone program around mcq_tabu3d_host for a sanitizer run of the HOST code of csrc/mcq_tabu3d.hip on a
// CPU: the shapes with one free cell, a repeated input, n_iters = 0, a refusal, and a run with every optional output.  No GPU is touched.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -o tabu3d_host_check \
//         tools/tabu3d_host_check.cpp monte-carlo-collective_amd/csrc/mcq_tabu3d.hip && ./tabu3d_host_check
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../include/mcq.h"

namespace {

int failures = 0;

void expect(bool ok, const char* what) {
    if (!ok) {
        std::printf("FAILED: %s (%s)\n", what, mcq_tabu3d_last_error());
        failures++;
    }
}

// the first Q cells of the cube in row-major order, but `skip` (a cell index, or -1)
std::vector<uint8_t> cube(int N, int Q, int skip) {
    std::vector<uint8_t> s;
    for (int c = 0; (int)s.size() < 3 * Q; c++) {
        if (c == skip) continue;
        s.push_back((uint8_t)(c / (N * N))), s.push_back((uint8_t)((c / N) % N)), s.push_back((uint8_t)(c % N));
    }
    return s;
}

struct Run {
    std::vector<uint8_t> out, best;
    std::vector<uint16_t> stamps;
    std::vector<int32_t> hist;
    int32_t e_in = -1, e_out = -1, b = -1, flags = -1;
    int64_t best_iter = -1, moves = -1, aspired = -1, uphill = -1, stalled = -1;
    int rc = 0;
};

Run run(int N, int Q, const std::vector<uint8_t>& in, long long iters, const std::vector<uint16_t>* tabu_in, int tenure, int tenure_rand, int tenure_conf) {
    Run r;
    const int C = N * N * N;
    r.out.assign(in.size(), 0), r.best.assign(in.size(), 0), r.stamps.assign((size_t)C, 0), r.hist.assign((size_t)iters + 1, -1);
    const uint32_t seed = 12345u;
    mcq_tabu3d q{};
    q.N = N, q.n_queens = Q, q.n_chains = 1, q.n_iters = iters, q.first_iter = (1ll << 32) - 3, q.tenure = tenure, q.tenure_rand = tenure_rand, q.tenure_conf = tenure_conf;
    q.seeds = &seed, q.state_in = in.data(), q.state_out = r.out.data(), q.best_state = r.best.data();
    q.tabu_in = tabu_in ? tabu_in->data() : nullptr, q.tabu_out = r.stamps.data();
    q.energy_in = &r.e_in, q.energy_out = &r.e_out, q.best_energy = &r.b, q.best_iter = &r.best_iter, q.flags = &r.flags;
    q.n_moves = &r.moves, q.n_aspired = &r.aspired, q.n_uphill = &r.uphill, q.n_stalled = &r.stalled;
    q.energy_hist = r.hist.data(), q.hist_stride = iters + 1;
    r.rc = mcq_tabu3d_host(&q);
    return r;
}

}  // namespace

int main() {
    for (int N = 2; N <= 4; N++) {  // one free cell, at the front, in the middle and at the end of the cube
        const int C = N * N * N;
        for (int skip : {0, C / 2, C - 1}) {
            const Run r = run(N, C - 1, cube(N, C - 1, skip), 50, nullptr, 3, 4, 10);
            expect(r.rc == MCQ_OK && r.flags == 0 && r.moves + r.stalled == 50 && r.hist[50] == r.e_out && r.b <= r.e_in, "one free cell");
        }
        std::vector<uint16_t> stamps((size_t)C);
        for (int c = 0; c < C; c++) stamps[(size_t)c] = (uint16_t)(65535 - c);
        const Run r = run(N, C - 2, cube(N, C - 2, 1), 40, &stamps, 8192, 4095, 64);
        expect(r.rc == MCQ_OK && r.moves + r.stalled == 40, "two free cells under the longest tenure and the latest stamps");
    }
    {  // a repeated input: queen 1 onto queen 0
        std::vector<uint8_t> s = cube(5, 25, -1);
        s[3] = s[0], s[4] = s[1], s[5] = s[2];
        const Run r = run(5, 25, s, 7, nullptr, 3, 0, 0);
        expect(r.rc == MCQ_OK && r.flags == MCQ_TABU3D_REPEATED && r.moves == 0 && r.out == s && r.best == s && r.hist[7] == r.e_in, "a repeated input");
    }
    for (int N : {2, 13, 20}) {  // n_iters = 0, with bytes above N - 1
        std::vector<uint8_t> s = cube(N, N * N, -1);
        s[2] = 255;
        const Run r = run(N, 0, s, 0, nullptr, 3, 0, 0);
        expect(r.rc == MCQ_OK && r.e_in == r.e_out && r.e_in == r.b && r.moves == 0 && r.stalled == 0 && r.out[2] == N - 1, "n_iters = 0");
    }
    {  // a walk in each of the other two shapes
        const Run a = run(13, 150, cube(13, 150, 7), 60, nullptr, 5, 5, 2), b = run(20, 401, cube(20, 401, 9), 30, nullptr, 5, 5, 2);
        expect(a.rc == MCQ_OK && a.moves == 60 && a.b < a.e_in && b.rc == MCQ_OK && b.moves == 30 && b.b < b.e_in, "N = 13 and N = 20");
    }
    {  // a refusal leaves the buffers alone
        const Run r = run(4, 64, cube(4, 63, -1), 3, nullptr, 3, 0, 0);
        expect(r.rc == MCQ_EINVAL && r.e_in == -1, "n_queens = N^3 is refused");
        expect(mcq_tabu3d_host(nullptr) == MCQ_EINVAL, "a NULL block is refused");
    }
    std::printf(failures ? "%d check(s) failed\n" : "tabu3d_host_check: all checks passed\n", failures);
    return failures != 0;
}
