"""The quench rule of include/mcq.h (mcq_quench) restated in NumPy, from the text of the rule and from nothing else: what
mcq_quench_host and the kernel are compared with, and the table the properties are checked on."""
import functools

import numpy as np


@functools.lru_cache(maxsize=None)
def _lines(N):
    """Per column c = i N + j: (flat indices of the other columns on its row, its column and its two diagonals, their d = max(|di|, |dj|))."""
    ii, jj = np.indices((N, N))
    out = []
    for i in range(N):
        for j in range(N):
            di, dj = np.abs(ii - i), np.abs(jj - j)
            on = ((di == 0) | (dj == 0) | (di == dj)) & ((di != 0) | (dj != 0))
            out.append((np.flatnonzero(on.ravel()), np.maximum(di, dj).ravel()[on.ravel()]))
    return out


def clamp(N, board):
    return np.minimum(np.asarray(board, dtype=np.int64).reshape(-1), N - 1)


def column(N, h, c):
    """a(c, k) for k = 0 .. N - 1 of the flat heights h (already clamped)."""
    idx, d = _lines(N)[c]
    diff = np.abs(h[idx][None, :] - np.arange(N)[:, None])
    return ((diff == 0) | (diff == d[None, :])).sum(axis=1)


def table(N, board):
    """a(c, k) as int64[N*N][N] of one board (clamped first)."""
    h = clamp(N, board)
    return np.stack([column(N, h, c) for c in range(N * N)])


def energy(N, board):
    h = clamp(N, board)
    two = int(table(N, h)[np.arange(N * N), h].sum())
    assert two % 2 == 0
    return two // 2


def quench(N, board, max_passes=0):
    """One board through the rule; returns a dict with the fields of mcq_quench plus `drops`, the energy differences of the moves."""
    h = clamp(N, board).copy()
    e_in = energy(N, h)
    E, moves, passes, drops = e_in, 0, 0, []
    while True:
        moved = 0
        for c in range(N * N):
            a = column(N, h, c)
            k = int(np.argmin(a))  # the first index of the minimum = the smallest k
            if a[k] < a[h[c]]:
                drops.append(int(a[h[c]] - a[k]))
                E -= drops[-1]
                h[c] = k
                moved += 1
        passes += 1
        moves += moved
        if moved == 0 or (max_passes > 0 and passes >= max_passes):
            break
    t = table(N, h)
    return {"state": h.astype(np.uint8), "energy_in": e_in, "energy_out": E, "n_moves": moves, "n_passes": passes,
            "conflicts": t[np.arange(N * N), h].astype(np.uint16), "drops": drops}


def is_local_minimum(N, board):
    """No column has a height with a lower count than the one it holds."""
    h = clamp(N, board)
    t = table(N, h)
    return bool((t.min(axis=1) == t[np.arange(N * N), h]).all())


def quench_many(N, states, max_passes=0):
    """quench over the rows of `states`, stacked like the library's outputs."""
    rows = [quench(N, s, max_passes) for s in np.asarray(states).reshape(-1, N * N)]
    out = {k: np.stack([np.asarray(r[k]) for r in rows]) for k in ("state", "energy_in", "energy_out", "n_moves", "n_passes", "conflicts")}
    out["drops"] = [r["drops"] for r in rows]
    return out


FIELDS = ("state", "energy_in", "energy_out", "n_moves", "n_passes", "conflicts")


def assert_equal(got, want, what):
    for k in FIELDS:
        np.testing.assert_array_equal(np.asarray(got[k]).astype(np.int64), np.asarray(want[k]).astype(np.int64), err_msg=f"{what}: {k}")


def random_boards(N, n, seed, over=False):
    """n random boards of edge N as uint8[n][N*N]; over=True mixes in bytes >= N (the library clamps them)."""
    rs = np.random.RandomState(seed)
    s = rs.randint(0, N, size=(n, N * N)).astype(np.uint8)
    if over:
        m = rs.random_sample(s.shape) < 0.1
        s[m] = rs.randint(N, 256, size=int(m.sum())).astype(np.uint8)
    return s


def klarner(N):
    """(3 i + 5 j) mod N: a zero-energy board where gcd(N, 210) = 1 (tests/golden/manifest.json: analytic.klarner_exact_board)."""
    i, j = np.indices((N, N))
    return ((3 * i + 5 * j) % N).astype(np.uint8).reshape(-1)
