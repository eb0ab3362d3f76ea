"""The full_3d quench rule of include/mcq.h (mcq_quench3d) restated in NumPy, from the text of the rule and from nothing else: what
mcq_quench3d_host and the kernel are compared with.  It is naive on purpose: an attack matrix of cells x queens rebuilt for every
visit, no attack field and no update shared with the library's approach."""
import functools

import numpy as np

FIELDS = ("state", "energy_in", "energy_out", "n_moves", "n_passes", "conflicts", "flags")


@functools.lru_cache(maxsize=None)
def _cells(N):
    """(i, j, k) of every cell in the order of the cell index i N^2 + j N + k, as int64[N^3][3]."""
    return np.stack(np.unravel_index(np.arange(N ** 3), (N, N, N)), axis=1).astype(np.int64)


def clamp(N, placement):
    """int64[Q][3] of one placement, every byte clamped to N - 1."""
    return np.minimum(np.asarray(placement, dtype=np.int64).reshape(-1, 3), N - 1)


def attack_matrix(targets, queens):
    """bool[T][Q]: the target cell is the queen's cell or attacks it -- the non-zero ones among |di|, |dj|, |dk| are all equal."""
    d = np.abs(targets[:, None, :] - queens[None, :, :])
    m = d.max(axis=2, keepdims=True)
    return ((d == 0) | (d == m)).all(axis=2)


def counts(N, queens, q, targets=None):
    """a(q, t) for every cell t (or the given cells) of the clamped placement `queens`: the queens q' != q that hold or attack t."""
    t = _cells(N) if targets is None else np.asarray(targets, dtype=np.int64).reshape(-1, 3)
    att = attack_matrix(t, queens)
    att[:, q] = False
    return att.sum(axis=1)


def held(N, queens):
    """a(q, pos(q)) for every queen."""
    att = attack_matrix(queens, queens)
    return att.sum(axis=1) - 1  # itself


def energy(N, placement):
    two = int(held(N, clamp(N, placement)).sum())
    assert two % 2 == 0
    return two // 2


def pairwise_energy(N, placement):
    """An independent recount: the seven predicates of the attack pair by pair, a plain double loop."""
    z = clamp(N, placement)
    E = 0
    for a in range(len(z)):
        for b in range(a + 1, len(z)):
            di, dj, dk = (abs(int(x)) for x in z[a] - z[b])
            E += (di == 0 and dj == 0) or (di == 0 and dk == 0) or (dj == 0 and dk == 0) or (dk == 0 and di == dj) or \
                 (dj == 0 and di == dk) or (di == 0 and dj == dk) or (di == dj == dk)
    return E


def is_repeated(N, placement):
    z = clamp(N, placement)
    return len(np.unique((z[:, 0] * N + z[:, 1]) * N + z[:, 2])) < len(z)


def quench(N, placement, max_passes=0):
    """One placement through the rule; returns a dict with the fields of mcq_quench3d."""
    z = clamp(N, placement).copy()
    Q = len(z)
    e_in = energy(N, z)
    E, moves, passes, flags = e_in, 0, 0, 0
    if is_repeated(N, z):
        flags = 1
    else:
        cells = _cells(N)
        att = attack_matrix(cells, z)  # cells x queens; a queen's column depends on that queen alone, so a move rewrites one column
        while True:
            moved = 0
            for q in range(Q):
                a = att.sum(axis=1, dtype=np.int64) - att[:, q]  # a(q, t) for every cell t
                idx = (z[:, 0] * N + z[:, 1]) * N + z[:, 2]
                now = int(a[idx[q]])
                a[np.delete(idx, q)] = a.max() + 1  # cells that hold another queen are no candidates
                t = int(np.argmin(a))  # the first index of the minimum = the smallest cell index
                if a[t] < now:
                    E += int(a[t]) - now
                    z[q] = cells[t]
                    att[:, q] = attack_matrix(cells, z[q:q + 1])[:, 0]
                    moved += 1
            passes += 1
            moves += moved
            if moved == 0 or (max_passes > 0 and passes >= max_passes):
                break
    return {"state": z.astype(np.uint8).reshape(-1), "energy_in": e_in, "energy_out": E, "n_moves": moves, "n_passes": passes,
            "conflicts": held(N, z).astype(np.uint16), "flags": flags}


def quench_many(N, states, Q=None, max_passes=0):
    """quench over the rows of `states`, stacked like the library's outputs."""
    Q = N * N if Q is None else Q
    rows = [quench(N, s, max_passes) for s in np.asarray(states).reshape(-1, 3 * Q)]
    return {k: np.stack([np.asarray(r[k]) for r in rows]) for k in FIELDS}


def is_local_minimum(N, placement):
    """No queen has a free cell with a lower count than the one it holds."""
    z = clamp(N, placement)
    idx = (z[:, 0] * N + z[:, 1]) * N + z[:, 2]
    for q in range(len(z)):
        a = counts(N, z, q)
        now = a[idx[q]]
        a[np.delete(idx, q)] = now
        if a.min() < now:
            return False
    return True


def assert_equal(got, want, what, fields=FIELDS):
    for k in fields:
        g, w = np.asarray(got[k]).astype(np.int64), np.asarray(want[k]).astype(np.int64)
        np.testing.assert_array_equal(g.reshape(w.shape), w, err_msg=f"{what}: {k}")


def random_placements(N, n, seed, Q=None, over=False):
    """n random placements of Q distinct cells as uint8[n][3 Q]; over=True raises bytes that equal N - 1 to values >= N here and
    there (the library clamps them back, so the cells stay distinct)."""
    Q = N * N if Q is None else Q
    rs = np.random.RandomState(seed)
    out = np.zeros((n, Q, 3), dtype=np.uint8)
    for r in range(n):
        flat = rs.choice(N ** 3, size=Q, replace=False)
        out[r] = np.stack([flat // (N * N), (flat // N) % N, flat % N], axis=1)
    if over:
        m = (out == N - 1) & (rs.random_sample(out.shape) < 0.3)
        out[m] = rs.randint(N, 256, size=int(m.sum())).astype(np.uint8)
    return out.reshape(n, 3 * Q)
