"""Weight rows and clocks a CALLER may hand to the n-fold entry points, which nfold.weight_tables and nfold.clock_tables never build
(their rows start at 2^24, never rise and are zero from the first zero on; their clocks are "exp" and "mean"), and the placement a chain
reaches under the row [1] and the clock of ones in closed form.  Every weight is at most B = 2^24, every row at most 128 (boards) or 512
(full_3d) wide, every clock entry at most 2^26: the bounds of include/mcq.h (mcq_nfold, mcq_nfold3d)."""
import functools

import numpy as np

from tests import nfold3d_util as n3
from tests import nfold_util as nu
from tests import quench3d_util as q3
from tests import quench_util as qu

B = 1 << 24
TIME_BITS = 12

SMALL = ("ones", "small", "up_only", "rising")  # weights of 1 to 8 where the differences are small: every U is on or next to a boundary
# W is of the order M 2^23 under these, tau = 1 under either clock of clocks() and a step fires up to 4096 events.  `clip` and `nonmono`
# climb until few rises are left and go quiet; `rand` and `altzero` never do
HEAVY = ("clip", "nonmono", "rand", "altzero")
NEVER_QUIET = ("rand", "altzero")


def rows(n_segs, width):
    """{name: uint32[n_segs][D]}, what each family reaches in csrc/mcq_nfold.hip and csrc/mcq_nfold3d.hip:
    ones      D = 1, [1]: W = M and every U is the first and the last integer of its move -- every comparison with U, u and the prefixes
    small     [2, 1, 0, 1]: non-monotone with a zero in the middle -- the same comparisons one integer inside a move, zero-weight moves
              between live ones
    up_only   [0, 1, 1, 1]: T[0] = 0, only rises carry weight and many R are 0 -- the chunk walk over R = 0 columns, `own != 0`
    only3     [0, 0, 0, 7, 0]: weight at one distance only
    rising    T[d] = d + 1 to the full width: strictly rising, so that every term of the 3-D kernel's corr(q) is negative (the uint64 sum
              wraps and comes back); wider than any difference, so the high clamp is `clip`'s, `small`'s and `nonmono`'s to reach
    clip      [1, B]: the high clamp d > D - 1 -> D - 1 lands on the largest weight
    nonmono   [3, B, 0, 5, 1]: T[0] != 2^24, a zero in the middle, the clamp on a small non-zero entry
    rand      D = 6, RandomState(5).randint(0, B + 1), a different row per segment: the per-segment restaging of T and of every R
    altzero   rows [B, 1000, 1] / [0, 0, 0] / [5, 0, B] in turn: a segment that sleeps between two live ones"""
    def rep(row):
        return np.tile(np.array([row], dtype=np.uint32), (n_segs, 1))

    alt = ([B, 1000, 1], [0, 0, 0], [5, 0, B])
    t = {"ones": rep([1]), "small": rep([2, 1, 0, 1]), "up_only": rep([0, 1, 1, 1]), "only3": rep([0, 0, 0, 7, 0]),
         "rising": rep(list(range(1, int(width) + 1))), "clip": rep([1, B]), "nonmono": rep([3, B, 0, 5, 1]),
         "rand": np.random.RandomState(5).randint(0, B + 1, size=(n_segs, 6)).astype(np.uint32),
         "altzero": np.array([alt[s % 3] for s in range(n_segs)], dtype=np.uint32).reshape(n_segs, 3)}
    assert all(v.dtype == np.uint32 and v.shape[0] == n_segs and 1 <= v.shape[1] <= width and int(v.max(initial=0)) <= B for v in t.values())
    return t


def clocks():
    """{name: (clock_ln2, uint32[256])}: "unit", l(x) = 1 whatever x is, and "exp16", the exponential clock at 2^4 instead of 2^24, whose
    last entries are 0 (need = 0 and tau = 1 occur with W > 0).  Small-weight rows fire about an event per step under them."""
    i = np.arange(256, dtype=np.float64)
    c = {"unit": (0, np.ones(256, dtype=np.uint32)),
         "exp16": (int(round(16 * np.log(2.0))), np.round(-16.0 * np.log((256.0 + i + 0.5) / 512.0)).astype(np.uint32))}
    assert c["exp16"][0] == 11 and int(c["exp16"][1].min()) == 0 and int(c["exp16"][1].max()) == 11
    return c


def aimed_need(weights, ticks):
    """The need with which a chain that carries the weights `weights` (one W per segment, of a placement that does not move) sleeps
    through every segment of one step but the last and fires its first event `ticks` units of 2^-12 step before the end of the last:
    each sleeping segment takes W off the need, and tau = floor(need 2^12 / W) of the last must be 2^12 - ticks."""
    *before, w_last = (int(w) for w in weights)
    assert w_last > 0 and 0 < ticks < 1 << TIME_BITS
    rest = -(-(((1 << TIME_BITS) - ticks) * w_last) >> TIME_BITS)  # the smallest need whose tau reaches 2^12 - ticks
    assert rest > 0 and (1 << TIME_BITS) - ticks <= ((rest << TIME_BITS) // w_last) < 1 << TIME_BITS
    return sum(before) + rest


def board_weights(N, board, tables):
    """W of `board` under every row of `tables`, from the restatement."""
    h = qu.clamp(N, board)
    return [int(nu.weights(N, h, row)[0].sum()) for row in np.asarray(tables)]


def queen_weights(N, placement, tables):
    """W of the placement under every row of `tables`, from the restatement."""
    z = q3.clamp(N, placement)
    return [int(n3.weights(N, z, row)[0].sum()) for row in np.asarray(tables)]


def _boards_after(N, boards, seeds, n):
    out = np.minimum(np.asarray(boards, dtype=np.int64).reshape(len(seeds), N * N), N - 1)
    M = N * N * (N - 1)
    cols = np.zeros((len(seeds), n), dtype=np.int64)
    for r, seed in enumerate(seeds):
        h = out[r]
        for e in range(n):
            x = nu.block(int(seed), e)
            U = ((((x[0] << 32) | x[1]) * M) >> 64)
            c, k = divmod(U, N - 1)
            h[c] = k + (k >= h[c])
            cols[r, e] = c
    return out.astype(np.uint8), cols


@functools.lru_cache(maxsize=None)
def _boards_checked():
    N, n = 3, 5
    s, seeds = qu.random_boards(N, 3, 1, over=True), np.array([7, 8, 4000000000], dtype=np.uint32)
    want = nu.nfold_many(N, s, seeds, rows(1, 128)["ones"], n, clocks()["unit"])
    assert (want["events_out"] == n).all() and (want["need_out"] == N * N * (N - 1)).all()
    assert (_boards_after(N, s, seeds, n)[0] == want["state"]).all()
    return True


def boards_after(N, boards, seeds, n):
    """(placements uint8[n_chains][N^2], moved columns int64[n_chains][n]) after n steps under the row [1] and the unit clock, from
    this file's imports of the restatement's Philox and from nothing in the library.  need = M = W, so tau is exactly one step and event e
    moves pair number U = (X_e M) >> 64 in the order c ascending, k ascending with k = h(c) skipped: c = U // (N - 1), and k is
    U % (N - 1) stepped past h(c).  Checked against nu.nfold at N = 3 on first use."""
    assert _boards_checked()
    return _boards_after(N, boards, seeds, n)


def _queens_after(N, Q, placements, seeds, n):
    out = np.minimum(np.asarray(placements, dtype=np.int64).reshape(len(seeds), Q, 3), N - 1)
    F = N ** 3 - Q
    drawn = np.zeros((len(seeds), n, 2), dtype=np.int64)
    for r, seed in enumerate(seeds):
        z = out[r]
        for e in range(n):
            x = n3.block(int(seed), e)
            U = ((((x[0] << 32) | x[1]) * (Q * F)) >> 64)
            q, i = divmod(U, F)
            t = i  # the i-th cell that holds no queen, in ascending order: every held cell at or below it moves it up by one
            for held in sorted(int(v) for v in n3.index_of(N, z)):
                if held > t:
                    break
                t += 1
            z[q] = (t // (N * N), (t // N) % N, t % N)
            drawn[r, e] = (q, t)
    return out.astype(np.uint8).reshape(len(seeds), 3 * Q), drawn


@functools.lru_cache(maxsize=None)
def _queens_checked():
    N, Q, n = 3, 4, 5
    s, seeds = q3.random_placements(N, 3, 1, Q=Q, over=True), np.array([7, 8, 4000000000], dtype=np.uint32)
    want = n3.nfold_many(N, s, seeds, rows(1, 512)["ones"], n, clocks()["unit"], Q=Q)
    assert (want["events_out"] == n).all() and (want["need_out"] == Q * (N ** 3 - Q)).all()
    assert (_queens_after(N, Q, s, seeds, n)[0] == want["state"]).all()
    return True


def queens_after(N, Q, placements, seeds, n):
    """(placements uint8[n_chains][3 Q], drawn (queen, cell) int64[n_chains][n][2]) after n steps under the row [1] and the unit clock:
    event e moves queen q = U // F to the cell free[U % F], U = (X_e M) >> 64, F = N^3 - Q and `free` the cells that hold no queen in
    ascending order.  Checked against n3.nfold at (N, Q) = (3, 4) on first use."""
    assert _queens_checked()
    return _queens_after(N, Q, placements, seeds, n)
