// relink3d_host_check.cpp -- a stand-alone program around mcq_relink3d_host for a sanitizer run of the HOST code of csrc/mcq_relink3d.hip
// on a CPU: the smallest cube, one with ragged Q and the largest, inputs with bytes >= N in the placement and in the guide, d0 = 0
// (the guide is the placement in another order) and d0 = Q (no cell shared), a cut walk, every optional output present and every one
// absent, in place, both repeats, and a refusal.  The host code works through pointers into its own vectors, its two lists and the
// caller's history rows; this run is what guards them.  No GPU is touched.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -o relink3d_host_check \
//         tools/relink3d_host_check.cpp monte-carlo-collective_amd/csrc/mcq_relink3d.hip && ./relink3d_host_check
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <vector>

#include "../include/mcq.h"

namespace {

int failures = 0;

void expect(bool ok, const char* what, int N, int Q) {
    if (!ok) {
        std::printf("FAILED: %s at N = %d, Q = %d (%s)\n", what, N, Q, mcq_relink3d_last_error());
        failures++;
    }
}

// a shuffle of the cube's cells from a small generator: the first Q are one placement, the next Q one that shares no cell with it
std::vector<int> shuffled_cells(int N, uint32_t x) {
    std::vector<int> c((size_t)(N * N * N));
    std::iota(c.begin(), c.end(), 0);
    for (size_t i = c.size() - 1; i > 0; i--) {
        x = x * 1664525u + 1013904223u;
        std::swap(c[i], c[(size_t)((x >> 8) % (uint32_t)(i + 1))]);
    }
    return c;
}

// n placements of Q cells each from `cells` (chain r takes them from offset `first`, rotated by r); bytes that equal N - 1 are raised
// to values >= N here and there (the entry points clamp them back, so the cells stay distinct)
std::vector<uint8_t> placements(int N, int Q, int n, const std::vector<int>& cells, size_t first, bool over) {
    std::vector<uint8_t> s((size_t)(3 * n * Q));
    for (int r = 0; r < n; r++)
        for (int q = 0; q < Q; q++) {
            const int c = cells[first + (size_t)((q + r) % Q)];
            uint8_t* t = &s[(size_t)(3 * (r * Q + q))];
            t[0] = (uint8_t)(c / (N * N)), t[1] = (uint8_t)((c / N) % N), t[2] = (uint8_t)(c % N);
            for (int x = 0; x < 3; x++)
                if (over && t[x] == N - 1 && (q + x) % 3 == 0) t[x] = (uint8_t)(N + (q * 7 + x) % (256 - N));
        }
    return s;
}

std::vector<uint8_t> clamped(std::vector<uint8_t> s, int N) {
    for (auto& b : s) b = b < N ? b : (uint8_t)(N - 1);
    return s;
}

bool in_cube(const std::vector<uint8_t>& s, int N) {
    for (uint8_t b : s)
        if (b >= N) return false;
    return true;
}

struct Run {
    std::vector<uint8_t> out, best;
    std::vector<int32_t> d0, steps, best_step, e_in, best_e, e_max, e_out, hist, flags;
    std::vector<int64_t> moves, passes;
    int rc = 0;
};

Run relink(int N, int Q, int n, const std::vector<uint8_t>& in, const std::vector<uint8_t>& guide, int max_steps, int min_dist, long long walk, bool optional) {
    Run r;
    const int W = max_steps ? max_steps : Q;
    r.out.assign(in.size(), 77), r.best.assign(in.size(), 78);
    for (auto* v : {&r.d0, &r.steps, &r.best_step, &r.e_in, &r.best_e, &r.e_max, &r.e_out, &r.flags}) v->assign((size_t)n, -1);
    r.moves.assign((size_t)n, -1), r.passes.assign((size_t)n, -1), r.hist.assign((size_t)(n * (W + 1)), -1);
    std::vector<uint32_t> seeds((size_t)n);
    for (int i = 0; i < n; i++) seeds[(size_t)i] = 0xFFFFFFF0u + (uint32_t)i * 7u;
    mcq_relink3d q{};
    q.N = N, q.n_queens = Q == N * N ? 0 : Q, q.n_chains = n, q.max_steps = max_steps, q.min_dist = min_dist, q.walk = walk;
    q.seeds = seeds.data(), q.state_in = in.data(), q.guide_in = guide.data(), q.state_out = r.out.data();
    if (optional) {
        q.path_best_state = r.best.data(), q.distance_in = r.d0.data(), q.n_steps = r.steps.data(), q.path_best_step = r.best_step.data();
        q.energy_in = r.e_in.data(), q.path_best_energy = r.best_e.data(), q.path_max_energy = r.e_max.data(), q.energy_out = r.e_out.data();
        q.n_moves = r.moves.data(), q.n_passes = r.passes.data(), q.energy_hist = r.hist.data(), q.hist_stride = W + 1, q.flags = r.flags.data();
    }
    r.rc = mcq_relink3d_host(&q);
    return r;
}

void shape(int N, int Q, int n) {
    const std::vector<int> cells = shuffled_cells(N, 11u + (uint32_t)(N * 131 + Q));
    const bool two = 2 * Q <= N * N * N;  // room for a placement that shares no cell
    const std::vector<uint8_t> a = placements(N, Q, n, cells, 0, true);
    // a guide that shares some cells: the placement's window of the shuffle moved by the room there is, at most Q / 2
    const size_t shift = (size_t)std::min(Q / 2 > 0 ? Q / 2 : 1, N * N * N - Q);
    const std::vector<uint8_t> g = placements(N, Q, n, cells, shift, true);
    const std::vector<int32_t> zeros((size_t)n, 0);

    const Run full = relink(N, Q, n, a, g, 0, 1, 0, true), slim = relink(N, Q, n, a, g, 0, 1, 0, false);
    expect(full.rc == MCQ_OK && slim.rc == MCQ_OK, "a walk between placements that share cells", N, Q);
    expect(full.out == slim.out && in_cube(full.out, N) && in_cube(full.best, N), "the placements with and without the optional outputs", N, Q);
    for (int r = 0; r < n; r++) {
        const size_t i = (size_t)r;
        expect(full.flags[i] == 0 && full.d0[i] == (int)shift && full.steps[i] == full.d0[i], "the distance", N, Q);
        expect(full.e_out[i] <= full.best_e[i] && full.best_e[i] <= full.e_max[i] && full.passes[i] >= 1, "the figures", N, Q);
        expect(full.hist[i * (size_t)(Q + 1)] == full.e_in[i] && full.hist[i * (size_t)(Q + 1) + (size_t)Q] >= 0, "the history's ends", N, Q);
    }
    // d0 = 0: the guide is the placement with its queens in another order
    std::vector<uint8_t> turned = a;
    for (int r = 0; r < n; r++) std::rotate(turned.begin() + 3 * r * Q, turned.begin() + 3 * r * Q + 3, turned.begin() + 3 * (r + 1) * Q);
    const Run same = relink(N, Q, n, a, turned, 0, 1, 5, true);
    expect(same.rc == MCQ_OK && same.d0 == zeros && same.steps == zeros && same.best == clamped(a, N), "d0 = 0", N, Q);
    if (two) {  // d0 = Q: no cell shared, and the guide a candidate
        const std::vector<uint8_t> far = placements(N, Q, n, cells, (size_t)Q, true);
        const Run all = relink(N, Q, n, a, far, 0, 0, (1ll << 40) + 3, true);
        expect(all.rc == MCQ_OK && all.d0 == std::vector<int32_t>((size_t)n, Q) && all.steps == all.d0, "d0 = Q", N, Q);
        const Run cut = relink(N, Q, n, a, far, 1, Q, 1, true);  // a cut walk and a window that holds nothing
        expect(cut.rc == MCQ_OK && cut.steps == std::vector<int32_t>((size_t)n, 1) && cut.best_step == zeros && cut.best == clamped(a, N), "max_steps = 1", N, Q);
    }
    // in place, without the optional outputs
    std::vector<uint8_t> io = a;
    std::vector<uint32_t> seeds((size_t)n, 1u);
    mcq_relink3d q{};
    q.N = N, q.n_queens = Q, q.n_chains = n, q.min_dist = 1;
    q.seeds = seeds.data(), q.state_in = io.data(), q.guide_in = g.data(), q.state_out = io.data();
    expect(mcq_relink3d_host(&q) == MCQ_OK && in_cube(io, N), "in place", N, Q);
    // both repeats: queen 1 onto queen 0, in the placement of chain 0 and in the guide of the last chain
    std::vector<uint8_t> ra = a, rg = g;
    std::copy(ra.begin(), ra.begin() + 3, ra.begin() + 3);
    std::copy(rg.begin() + 3 * (n - 1) * Q, rg.begin() + 3 * (n - 1) * Q + 3, rg.begin() + 3 * (n - 1) * Q + 3);
    const Run rep = relink(N, Q, n, ra, rg, 0, 1, 0, true), rep_slim = relink(N, Q, n, ra, rg, 2 <= Q ? 2 : 1, 1, 0, false);
    expect(rep.rc == MCQ_OK && rep_slim.rc == MCQ_OK, "repeated inputs", N, Q);
    expect((rep.flags[0] & MCQ_RELINK3D_REPEATED) && (rep.flags[(size_t)n - 1] & MCQ_RELINK3D_GUIDE_REPEATED), "the repeat flags", N, Q);
    expect(rep.d0[0] == 0 && rep.moves[0] == 0 && rep.passes[0] == 0 && rep.e_in[0] == rep.e_out[0] && rep.hist[(size_t)Q] == rep.e_in[0], "a repeated chain is handed back", N, Q);
    expect(std::equal(rep.out.begin(), rep.out.begin() + 3 * Q, clamped(ra, N).begin()), "a repeated chain's placement", N, Q);
}

}  // namespace

int main() {
    shape(2, 4, 3);
    shape(2, 7, 2);
    shape(5, 25, 3);
    shape(5, 77, 2);
    shape(5, 124, 2);
    shape(32, 1024, 1);
    shape(32, 300, 2);
    const std::vector<int> cells = shuffled_cells(5, 3u);
    const std::vector<uint8_t> a = placements(5, 25, 1, cells, 0, false);
    std::vector<uint8_t> o = a;
    mcq_relink3d q{};
    uint32_t seed = 1;
    q.N = 5, q.n_chains = 1, q.min_dist = 1;
    q.seeds = &seed, q.state_in = a.data(), q.guide_in = o.data(), q.state_out = o.data();
    if (mcq_relink3d_host(&q) != MCQ_EINVAL || !std::strstr(mcq_relink3d_last_error(), "guide_in")) {
        std::printf("FAILED: a state_out that is guide_in was not refused\n");
        failures++;
    }
    q.N = 33;
    if (mcq_relink3d_host(&q) != MCQ_EINVAL || mcq_relink3d_host(nullptr) != MCQ_EINVAL) {
        std::printf("FAILED: N = 33 or a NULL block was not refused\n");
        failures++;
    }
    q.N = 5, q.max_steps = 26;
    if (mcq_relink3d_host(&q) != MCQ_EINVAL) {
        std::printf("FAILED: max_steps above Q was not refused\n");
        failures++;
    }
    if (failures) std::printf("relink3d_host_check: %d failure(s)\n", failures);
    else std::printf("relink3d_host_check: clean\n");
    return failures ? 1 : 0;
}
