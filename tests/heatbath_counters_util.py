"""The counter form of the heat-bath column sweep (include/mcq.h: mcq_heatbath_counters_device) restated in NumPy from the identity the
header gives and from nothing else: the 12 line families of the cube with in-plane direction (0,1), (1,0), (1,1), (1,-1) and height step
0, +1, -1 per cell, one queen counter per line, a(c, k) as the sum of the 12 counters of the lines through (i, j, k) minus 12 [k = h(c)],
and a height change as 12 decrements and 12 increments.  A line is named by what its cells share, not by where a kernel keeps it."""
import numpy as np

from tests import quench_util as qu

DIRECTIONS = ((0, 1), (1, 0), (1, 1), (1, -1))
STEPS = (0, 1, -1)
FAMILIES = tuple((d, s) for d in DIRECTIONS for s in STEPS)


def line(N, f, i, j, k):
    """The line of family f through the cell (i, j, k), as an index pair into an int array [3N][3N]: (what the in-plane line keeps,
    what the height keeps along it), both shifted by N so that neither is negative."""
    (di, dj), s = FAMILIES[f]
    if (di, dj) == (0, 1):
        plane, pos = i, j
    elif (di, dj) == (1, 0):
        plane, pos = j, i
    elif (di, dj) == (1, 1):
        plane, pos = i - j, i
    else:
        plane, pos = i + j, i
    return plane + N, k - s * pos + N


def build(N, board):
    """The counters int64[12][3N][3N] of a board (clamped first)."""
    h = qu.clamp(N, board)
    cnt = np.zeros((12, 3 * N, 3 * N), dtype=np.int64)
    for c in range(N * N):
        for f in range(12):
            cnt[(f,) + line(N, f, c // N, c % N, int(h[c]))] += 1
    return cnt


def table(N, cnt, h):
    """a(c, k) as int64[N*N][N] from the counters and the (clamped) heights."""
    a = np.zeros((N * N, N), dtype=np.int64)
    for c in range(N * N):
        for k in range(N):
            a[c, k] = sum(int(cnt[(f,) + line(N, f, c // N, c % N, k)]) for f in range(12)) - (12 if k == int(h[c]) else 0)
    return a


def change(N, cnt, h, c, k_new):
    """Column c of the heights h takes the height k_new (different from the one it holds), in place: 12 decrements on the lines through
    the old cell and 12 increments on the lines through the new one.  Returns the 24 counters touched."""
    i, j, k_old = c // N, c % N, int(h[c])
    assert k_new != k_old
    touched = []
    for f in range(12):
        old, new = (f,) + line(N, f, i, j, k_old), (f,) + line(N, f, i, j, k_new)
        cnt[old] -= 1
        cnt[new] += 1
        touched += [old, new]
    h[c] = k_new
    return touched


def n_lines(N):
    """The number of distinct lines of the 12 families that hold a cell of the cube."""
    seen = set()
    for i in range(N):
        for j in range(N):
            for k in range(N):
                seen.update((f,) + line(N, f, i, j, k) for f in range(12))
    return len(seen)


def special_boards(N):
    """h = (i + j) mod N and h = i: boards that fill whole diagonal lines, so a counter reaches N."""
    i, j = np.indices((N, N))
    return ((i + j) % N).astype(np.uint8).reshape(-1), (i + 0 * j).astype(np.uint8).reshape(-1)
