// relink_host_check.cpp -- a stand-alone program around mcq_relink_host for a sanitizer run of the HOST code of csrc/mcq_relink.hip on a
// CPU: the smallest board, one where N is no multiple of 4 and the largest, inputs with bytes >= N in the placement and in the guide,
// d0 = 0 and d0 = N^2, a cut walk, every optional output present and every one absent, both local searches, and a refusal.  The host
// code works through pointers into its own vectors and the caller's history rows; this run is what guards them.  No GPU is touched.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -o relink_host_check \
//         tools/relink_host_check.cpp monte-carlo-collective_amd/csrc/mcq_relink.hip && ./relink_host_check
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../include/mcq.h"

namespace {

int failures = 0;

void expect(bool ok, const char* what, int N) {
    if (!ok) {
        std::printf("FAILED: %s at N = %d (%s)\n", what, N, mcq_relink_last_error());
        failures++;
    }
}

// n boards of N^2 bytes from a small generator, a few of them >= N (the entry points clamp them to N - 1)
std::vector<uint8_t> boards(int N, int n, uint32_t x) {
    std::vector<uint8_t> s((size_t)(n * N * N));
    for (auto& b : s) {
        x = x * 1664525u + 1013904223u;
        b = (uint8_t)((x >> 16) % (unsigned)N);
    }
    s[0] = 255, s[s.size() - 1] = (uint8_t)N, s[s.size() / 2] = 200;
    return s;
}

std::vector<uint8_t> clamped(std::vector<uint8_t> s, int N) {
    for (auto& b : s) b = b < N ? b : (uint8_t)(N - 1);
    return s;
}

struct Run {
    std::vector<uint8_t> out, best;
    std::vector<int32_t> d0, steps, best_step, e_in, best_e, e_max, e_out, hist;
    std::vector<int64_t> moves, pair_moves;
    int rc = 0;
};

Run relink(int N, int n, const std::vector<uint8_t>& in, const std::vector<uint8_t>& guide, int max_steps, int min_dist, int search, long long walk,
           bool optional) {
    Run r;
    const int W = max_steps ? max_steps : N * N;
    r.out.assign(in.size(), 77), r.best.assign(in.size(), 78);
    for (auto* v : {&r.d0, &r.steps, &r.best_step, &r.e_in, &r.best_e, &r.e_max, &r.e_out}) v->assign((size_t)n, -1);
    r.moves.assign((size_t)n, -1), r.pair_moves.assign((size_t)n, -1), r.hist.assign((size_t)(n * (W + 1)), -1);
    std::vector<uint32_t> seeds((size_t)n);
    for (int i = 0; i < n; i++) seeds[(size_t)i] = 0xFFFFFFF0u + (uint32_t)i * 7u;
    mcq_relink q{};
    q.N = N, q.mode = MCQ_MODE_BOARD, q.n_chains = n, q.max_steps = max_steps, q.min_dist = min_dist, q.local_search = search, q.walk = walk;
    q.seeds = seeds.data(), q.state_in = in.data(), q.guide_in = guide.data(), q.state_out = r.out.data();
    if (optional) {
        q.path_best_state = r.best.data(), q.distance_in = r.d0.data(), q.n_steps = r.steps.data(), q.path_best_step = r.best_step.data();
        q.energy_in = r.e_in.data(), q.path_best_energy = r.best_e.data(), q.path_max_energy = r.e_max.data(), q.energy_out = r.e_out.data();
        q.n_moves = r.moves.data(), q.n_pair_moves = r.pair_moves.data(), q.energy_hist = r.hist.data(), q.hist_stride = W + 1;
    }
    r.rc = mcq_relink_host(&q);
    return r;
}

bool on_board(const std::vector<uint8_t>& s, int N) {
    for (uint8_t b : s)
        if (b >= N) return false;
    return true;
}

void shape(int N) {
    const int n = 3, Q = N * N;
    const std::vector<uint8_t> a = boards(N, n, 11u + (uint32_t)N), g = boards(N, n, 97u + (uint32_t)N);
    for (int search : {MCQ_HOP_SINGLE, MCQ_HOP_PAIRS}) {
        const Run full = relink(N, n, a, g, 0, 1, search, 0, true), slim = relink(N, n, a, g, 0, 1, search, 0, false);
        expect(full.rc == MCQ_OK && slim.rc == MCQ_OK, "a walk between random boards", N);
        expect(full.out == slim.out && on_board(full.out, N) && on_board(full.best, N), "the placements with and without the optional outputs", N);
        for (int r = 0; r < n; r++) {
            const size_t i = (size_t)r;
            expect(full.steps[i] == full.d0[i] && full.d0[i] <= Q && full.e_out[i] <= full.best_e[i] && full.best_e[i] <= full.e_max[i], "the figures", N);
            expect(full.hist[i * (size_t)(Q + 1)] == full.e_in[i] && full.hist[i * (size_t)(Q + 1) + (size_t)Q] >= 0, "the history's ends", N);
        }
        // d0 = 0: the guide is the placement
        const Run same = relink(N, n, a, a, 0, 1, search, 5, true);
        expect(same.rc == MCQ_OK && same.d0 == std::vector<int32_t>((size_t)n, 0) && same.best == clamped(a, N), "d0 = 0", N);
        // d0 = N^2: every column one height off, and the guide a candidate
        std::vector<uint8_t> off = clamped(a, N);
        for (auto& b : off) b = (uint8_t)((b + 1) % N);
        const Run all = relink(N, n, a, off, 0, 0, search, (1ll << 40) + 3, true);
        expect(all.rc == MCQ_OK && all.d0 == std::vector<int32_t>((size_t)n, Q) && all.steps == all.d0, "d0 = N^2", N);
        // a cut walk, a window that holds nothing, in place
        Run cut = relink(N, n, a, off, 1, Q, search, 1, true);
        expect(cut.rc == MCQ_OK && cut.steps == std::vector<int32_t>((size_t)n, 1) && cut.best_step == std::vector<int32_t>((size_t)n, 0), "max_steps = 1", N);
        std::vector<uint8_t> io = a;
        mcq_relink q{};
        std::vector<uint32_t> seeds((size_t)n, 1u);
        q.N = N, q.mode = MCQ_MODE_BOARD, q.n_chains = n, q.min_dist = 1, q.local_search = search;
        q.seeds = seeds.data(), q.state_in = io.data(), q.guide_in = g.data(), q.state_out = io.data();
        expect(mcq_relink_host(&q) == MCQ_OK && on_board(io, N), "in place", N);
    }
}

}  // namespace

int main() {
    for (int N : {2, 5, 32}) shape(N);
    const std::vector<uint8_t> a = boards(5, 1, 1u);
    std::vector<uint8_t> o = a;
    mcq_relink q{};
    uint32_t seed = 1;
    q.N = 5, q.mode = MCQ_MODE_BOARD, q.n_chains = 1, q.min_dist = 1, q.local_search = MCQ_HOP_PAIRS;
    q.seeds = &seed, q.state_in = a.data(), q.guide_in = o.data(), q.state_out = o.data();
    if (mcq_relink_host(&q) != MCQ_EINVAL || !std::strstr(mcq_relink_last_error(), "guide_in")) {
        std::printf("FAILED: a state_out that is guide_in was not refused\n");
        failures++;
    }
    q.N = 33;
    if (mcq_relink_host(&q) != MCQ_EINVAL || mcq_relink_host(nullptr) != MCQ_EINVAL) {
        std::printf("FAILED: N = 33 or a NULL block was not refused\n");
        failures++;
    }
    if (failures) std::printf("relink_host_check: %d failure(s)\n", failures);
    else std::printf("relink_host_check: clean\n");
    return failures ? 1 : 0;
}
