"""The pair-move quench rule of include/mcq.h (mcq_quench_pairs) restated in NumPy from the text of the rule, on top of
tests/quench_util.py: what mcq_quench_pairs_host and the kernel are compared with.  The scan here goes over ALL pairs of columns,
aligned or not, and skips no candidate; for N <= 4 it takes D from a full recount of the energy instead of the formula.  It is
therefore independent of both shortcuts the library may take."""
import functools

import numpy as np

from tests import quench_util as qu

FIELDS = ("state", "energy_in", "energy_single", "energy_out", "n_moves", "n_pair_moves", "n_rounds", "certified", "conflicts")
RECOUNT_MAX_N = 4


@functools.lru_cache(maxsize=None)
def geometry(N):
    """(aligned bool[Q][Q], d int64[Q][Q]) over the row-major columns: rule item 1."""
    i, j = np.divmod(np.arange(N * N), N)
    di, dj = np.abs(i[:, None] - i[None, :]), np.abs(j[:, None] - j[None, :])
    aligned = ((di == 0) | (dj == 0) | (di == dj)) & ((di != 0) | (dj != 0))
    return aligned, np.maximum(di, dj)


def recount(N, boards):
    """E of each row of `boards` (int64[M][Q], clamped) from the definition: attacking pairs of aligned columns, each counted once."""
    aligned, d = geometry(N)
    b = np.asarray(boards, dtype=np.int64).reshape(-1, N * N)
    diff = np.abs(b[:, :, None] - b[:, None, :])
    two = (aligned[None] & ((diff == 0) | (diff == d[None]))).sum(axis=(1, 2))
    assert (two % 2 == 0).all()
    return two // 2


def att(N, c1, k1, c2, k2):
    """att((c1, k1), (c2, k2)); k1 and k2 may be arrays."""
    aligned, d = geometry(N)
    x = np.abs(np.asarray(k1) - np.asarray(k2))
    return (bool(aligned[c1, c2]) & ((x == 0) | (x == d[c1, c2]))).astype(np.int64)


def pair_deltas(N, h, c1, c2, delta="formula", t=None):
    """D of every (k1, k2) of the pair c1 < c2 as int64[N][N]; the entries with k1 = h(c1) or k2 = h(c2) are no candidates."""
    k = np.arange(N)
    if delta == "recount":
        b = np.repeat(h[None, :], N * N, axis=0)
        b[:, c1], b[:, c2] = np.repeat(k, N), np.tile(k, N)
        return (recount(N, b) - recount(N, h[None])[0]).reshape(N, N)
    t = qu.table(N, h) if t is None else t
    h1, h2 = h[c1], h[c2]
    return (t[c1][:, None] - t[c1][h1] + t[c2][None, :] - t[c2][h2]
            - att(N, c1, k, c2, h2)[:, None] - att(N, c1, h1, c2, k)[None, :] + att(N, c1, h1, c2, h2) + att(N, c1, k[:, None], c2, k[None, :]))


def scan(N, h, pairs="all", delta=None):
    """The lexicographically smallest (D, c1, c2, k1, k2) over the candidates: rule item 3.  pairs="all" visits every pair of columns,
    "aligned" only the aligned ones; delta is "formula" or "recount" (default: recount up to N = RECOUNT_MAX_N)."""
    delta = delta or ("recount" if N <= RECOUNT_MAX_N else "formula")
    aligned, _ = geometry(N)
    t = qu.table(N, h) if delta == "formula" else None
    best = None
    for c1 in range(N * N):
        for c2 in range(c1 + 1, N * N):
            if pairs == "aligned" and not aligned[c1, c2]:
                continue
            D = pair_deltas(N, h, c1, c2, delta, t).astype(np.int64)
            big = np.iinfo(np.int64).max
            D[h[c1], :] = big
            D[:, h[c2]] = big
            m = int(D.min())
            k1, k2 = np.argwhere(D == m)[0]  # row-major: the smallest (k1, k2)
            cand = (m, c1, c2, int(k1), int(k2))
            if best is None or cand < best:
                best = cand
    return best


def descend(N, h):
    """Passes of the single-move rule until one moves nothing; returns (heights, energy drop, moves)."""
    r = qu.quench(N, h)
    return r["state"].astype(np.int64), r["energy_in"] - r["energy_out"], r["n_moves"]


def quench_pairs(N, board, max_rounds=0, pairs="all", delta=None):
    """One board through the rule; returns a dict with the fields of mcq_quench_pairs plus `deltas`, the D of the pair moves."""
    h = qu.clamp(N, board).copy()
    e_in = qu.energy(N, h)
    h, drop, moves = descend(N, h)
    E = e_single = e_in - drop
    rounds = pair_moves = certified = 0
    deltas = []
    while True:
        rounds += 1
        D, c1, c2, k1, k2 = scan(N, h, pairs, delta)
        if D >= 0:
            certified = 1
            break
        h[c1], h[c2] = k1, k2
        E += D
        deltas.append(D)
        pair_moves += 1
        h, drop, m = descend(N, h)
        E -= drop
        moves += m
        if max_rounds > 0 and rounds >= max_rounds:
            break
    t = qu.table(N, h)
    return {"state": h.astype(np.uint8), "energy_in": e_in, "energy_single": e_single, "energy_out": E, "n_moves": moves,
            "n_pair_moves": pair_moves, "n_rounds": rounds, "certified": certified,
            "conflicts": t[np.arange(N * N), h].astype(np.uint16), "deltas": deltas}


def quench_pairs_many(N, states, max_rounds=0, **kw):
    rows = [quench_pairs(N, s, max_rounds, **kw) for s in np.asarray(states).reshape(-1, N * N)]
    out = {k: np.stack([np.asarray(r[k]) for r in rows]) for k in FIELDS}
    out["deltas"] = [r["deltas"] for r in rows]
    return out


def assert_equal(got, want, what):
    for k in FIELDS:
        np.testing.assert_array_equal(np.asarray(got[k]).astype(np.int64), np.asarray(want[k]).astype(np.int64), err_msg=f"{what}: {k}")


def has_improving_pair_by_recount(N, board):
    h = qu.clamp(N, board)
    return scan(N, h, "all", "recount")[0] < 0
