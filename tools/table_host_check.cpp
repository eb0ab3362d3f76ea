// table_host_check.cpp -- a stand-alone program around mcq_quench_pairs_host, mcq_hop_host and mcq_tabu_host for a sanitizer run of the HOST
// code of csrc/mcq_table.h and of the three files on it, on a CPU: the smallest board, one where N is no multiple of 4 and the largest,
// inputs with bytes >= N, n_hops = 0 and n_iters = 0, every optional output present and every one absent, and a refusal per entry point.
// The shared host code works through pointers into its callers' vectors; this run is what guards them.  No GPU is touched.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -o table_host_check \
//         tools/table_host_check.cpp monte-carlo-collective_amd/csrc/mcq_quench_pairs.hip monte-carlo-collective_amd/csrc/mcq_hop.hip \
//         monte-carlo-collective_amd/csrc/mcq_tabu.hip && ./table_host_check
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../include/mcq.h"

namespace {

int failures = 0;

void expect(bool ok, const char* what, int N, const char* err) {
    if (!ok) {
        std::printf("FAILED: %s at N = %d (%s)\n", what, N, err);
        failures++;
    }
}

// a board of N^2 bytes from a small generator, a few of them >= N (the entry points clamp them to N - 1)
std::vector<uint8_t> board(int N, uint32_t x) {
    std::vector<uint8_t> s((size_t)(N * N));
    for (auto& b : s) {
        x = x * 1664525u + 1013904223u;
        b = (uint8_t)((x >> 16) % (unsigned)N);
    }
    s[0] = 255, s[s.size() - 1] = (uint8_t)N, s[s.size() / 2] = 200;
    return s;
}

bool on_board(const std::vector<uint8_t>& s, int N) {
    for (uint8_t b : s)
        if (b >= N) return false;
    return true;
}

struct Pairs {
    std::vector<uint8_t> out;
    std::vector<uint16_t> conflicts;
    int32_t e_in = -1, e_single = -1, e_out = -1, moves = -1, pair_moves = -1, rounds = -1, certified = -1;
    int rc = 0;
};

Pairs pairs(int N, const std::vector<uint8_t>& in, long long max_rounds, bool optional) {
    Pairs r;
    r.out.assign(in.size(), 77), r.conflicts.assign(in.size(), 0);
    mcq_quench_pairs q{};
    q.N = N, q.n_chains = 1, q.max_rounds = max_rounds, q.state_in = in.data(), q.state_out = r.out.data();
    if (optional) {
        q.energy_in = &r.e_in, q.energy_single = &r.e_single, q.energy_out = &r.e_out, q.n_moves = &r.moves, q.n_pair_moves = &r.pair_moves;
        q.n_rounds = &r.rounds, q.certified = &r.certified, q.conflicts = r.conflicts.data();
    }
    r.rc = mcq_quench_pairs_host(&q);
    return r;
}

struct Hop {
    std::vector<uint8_t> out, best;
    std::vector<int32_t> hist;
    int32_t e_in = -1, e_start = -1, e_out = -1, b = -1;
    int64_t best_hop = -1, accepted = -1, improved = -1, moves = -1, pair_moves = -1;
    int rc = 0;
};

Hop hop(int N, const std::vector<uint8_t>& in, long long n_hops, int local_search, bool optional) {
    Hop r;
    r.out.assign(in.size(), 77), r.best.assign(in.size(), 77), r.hist.assign((size_t)n_hops + 1, -1);
    const uint32_t seed = 4321u;
    mcq_hop q{};
    q.N = N, q.n_chains = 1, q.n_hops = n_hops, q.first_hop = (1ll << 33) - 1, q.kick = 3, q.slack = 1, q.local_search = local_search;
    q.seeds = &seed, q.state_in = in.data(), q.state_out = r.out.data();
    if (optional) {
        q.energy_in = &r.e_in, q.energy_start = &r.e_start, q.energy_out = &r.e_out, q.best_energy = &r.b, q.best_hop = &r.best_hop;
        q.best_state = r.best.data(), q.n_accepted = &r.accepted, q.n_improved = &r.improved, q.n_moves = &r.moves, q.n_pair_moves = &r.pair_moves;
        q.energy_hist = r.hist.data(), q.hist_stride = n_hops + 1;
    }
    r.rc = mcq_hop_host(&q);
    return r;
}

struct Tabu {
    std::vector<uint8_t> out, best;
    std::vector<uint16_t> stamps;
    std::vector<int32_t> hist;
    int32_t e_in = -1, e_out = -1, b = -1;
    int64_t best_iter = -1, moves = -1, aspired = -1, uphill = -1, stalled = -1;
    int rc = 0;
};

Tabu tabu(int N, const std::vector<uint8_t>& in, long long iters, bool optional) {
    Tabu r;
    r.out.assign(in.size(), 77), r.best.assign(in.size(), 77), r.stamps.assign((size_t)(N * N * N), 0), r.hist.assign((size_t)iters + 1, -1);
    std::vector<uint16_t> tabu_in((size_t)(N * N * N));
    for (size_t e = 0; e < tabu_in.size(); e++) tabu_in[e] = (uint16_t)(e % 7 == 0 ? 65535 - e : 0);
    const uint32_t seed = 12345u;
    const int32_t floor = 1 << 20;
    mcq_tabu q{};
    q.N = N, q.n_chains = 1, q.n_iters = iters, q.first_iter = (1ll << 32) - 3, q.tenure = 3, q.tenure_rand = 4, q.tenure_conf = 10;
    q.seeds = &seed, q.state_in = in.data(), q.state_out = r.out.data();
    if (optional) {
        q.tabu_in = tabu_in.data(), q.tabu_out = r.stamps.data(), q.best_floor = &floor, q.best_state = r.best.data();
        q.energy_in = &r.e_in, q.energy_out = &r.e_out, q.best_energy = &r.b, q.best_iter = &r.best_iter;
        q.n_moves = &r.moves, q.n_aspired = &r.aspired, q.n_uphill = &r.uphill, q.n_stalled = &r.stalled;
        q.energy_hist = r.hist.data(), q.hist_stride = iters + 1;
    }
    r.rc = mcq_tabu_host(&q);
    return r;
}

}  // namespace

int main() {
    for (int N : {2, 5, 32}) {
        const std::vector<uint8_t> in = board(N, 17u * (unsigned)N);
        std::vector<uint8_t> clamped_in = in;
        for (auto& b : clamped_in) b = b < N ? b : (uint8_t)(N - 1);
        {
            const Pairs a = pairs(N, in, 0, true), b = pairs(N, in, 0, false);
            const char* err = mcq_quench_pairs_last_error();
            expect(a.rc == MCQ_OK && b.rc == MCQ_OK && a.out == b.out && on_board(a.out, N), "the pair quench with and without its optional outputs", N, err);
            expect(a.e_out <= a.e_single && a.e_single <= a.e_in && a.rounds >= 1 && a.certified == 1, "the pair quench's figures", N, err);
            long twoE = 0;
            for (uint16_t c : a.conflicts) twoE += c;
            expect(twoE == 2l * a.e_out, "conflicts add up to 2 energy_out", N, err);
            const Hop h0 = hop(N, in, 0, MCQ_HOP_PAIRS, true);  // n_hops = 0 is the local search alone
            expect(h0.rc == MCQ_OK && h0.out == a.out && h0.best == a.out && h0.e_in == a.e_in && h0.e_start == a.e_out && h0.hist[0] == a.e_out &&
                       h0.moves == a.moves && h0.pair_moves == a.pair_moves && h0.accepted == 0,
                   "n_hops = 0 is the pair quench", N, mcq_hop_last_error());
        }
        for (int ls : {MCQ_HOP_SINGLE, MCQ_HOP_PAIRS}) {
            const long long n = 6;
            const Hop a = hop(N, in, n, ls, true), b = hop(N, in, n, ls, false);
            const char* err = mcq_hop_last_error();
            expect(a.rc == MCQ_OK && b.rc == MCQ_OK && a.out == b.out && on_board(a.out, N) && on_board(a.best, N), "hops with and without their optional outputs", N, err);
            expect(a.hist[0] == a.e_start && a.hist[(size_t)n] == a.e_out && a.b <= a.e_start && a.e_start <= a.e_in && a.accepted <= n &&
                       (ls == MCQ_HOP_PAIRS || a.pair_moves == 0),
                   "the hops' figures", N, err);
            if (ls == MCQ_HOP_SINGLE) expect(hop(N, in, 0, ls, true).rc == MCQ_OK, "n_hops = 0 with single moves", N, mcq_hop_last_error());
        }
        {
            const long long n = 50;
            const Tabu a = tabu(N, in, n, true), b = tabu(N, in, n, false), z = tabu(N, in, 0, true);
            const char* err = mcq_tabu_last_error();
            expect(a.rc == MCQ_OK && b.rc == MCQ_OK && on_board(a.out, N) && on_board(b.out, N) && on_board(a.best, N), "tabu search with and without its optional outputs", N, err);
            expect(a.moves + a.stalled == n && a.hist[(size_t)n] == a.e_out && a.b <= a.e_in && a.uphill <= a.moves, "tabu search's figures", N, err);
            expect(z.rc == MCQ_OK && z.out == clamped_in && z.best == clamped_in && z.e_in == z.e_out && z.moves == 0 && z.stalled == 0 && z.hist[0] == z.e_in,
                   "n_iters = 0 is the recount", N, err);
        }
    }
    {  // a refusal per entry point leaves the buffers alone
        const std::vector<uint8_t> in = board(5, 3u);
        const Pairs p = pairs(5, in, -1, true);
        expect(p.rc == MCQ_EINVAL && p.e_in == -1 && p.out[0] == 77, "a negative max_rounds is refused", 5, mcq_quench_pairs_last_error());
        const Hop h = hop(5, in, 2, 2, true);
        expect(h.rc == MCQ_EINVAL && h.e_in == -1 && h.out[0] == 77, "a local_search that is neither value is refused", 5, mcq_hop_last_error());
        const Tabu t = tabu(33, board(33, 3u), 2, true);
        expect(t.rc == MCQ_EINVAL && t.e_in == -1 && t.out[0] == 77, "N = 33 is refused", 33, mcq_tabu_last_error());
        expect(mcq_quench_pairs_host(nullptr) == MCQ_EINVAL && mcq_hop_host(nullptr) == MCQ_EINVAL && mcq_tabu_host(nullptr) == MCQ_EINVAL, "a NULL block is refused", 0, "");
    }
    std::printf(failures ? "%d check(s) failed\n" : "table_host_check: all checks passed\n", failures);
    return failures != 0;
}
