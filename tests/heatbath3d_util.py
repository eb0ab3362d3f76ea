"""The full_3d heat-bath rule of include/mcq.h (mcq_heatbath3d) restated in NumPy and Python integers, from the text of the rule and from
nothing else.  a(q, t) is tests/quench3d_util.counts, which tests/golden/conflicts_3d.npz pins to the reference; Philox and the weight
table are those of tests/heatbath_util.py; x W >> 64 is a Python integer.  It is naive on purpose: the counts of all cells are rebuilt
from the placement for every update, no attack field, no update shared with the library's approach."""
import functools

import numpy as np

from tests import heatbath_util as hu
from tests import quench3d_util as q3

FIELDS = ("state", "energy_in", "energy_out", "best_energy", "best_sweep", "best_state", "n_changed", "flags")
MASK = 0xFFFFFFFF


def word(seed, w):
    """Word w (a Python integer below 2^63) of the full_3d heat-bath stream of a chain seeded `seed`: key word 2."""
    b = w >> 2
    return hu.philox((b & MASK, b >> 32, 0, 0), (seed, 2))[w & 3]


def draw(seed, u):
    """x of update u = g Q + q: the words 2 u and 2 u + 1."""
    return word(seed, 2 * u) | word(seed, 2 * u + 1) << 32


def cell_index(N, z):
    return (z[:, 0] * N + z[:, 1]) * N + z[:, 2]


def sweeps(N, placement, seed, tab, n_sweeps, first_sweep=0):
    """One chain through the rule with the rows tab[0 .. n_sweeps - 1]; returns a dict with the fields of mcq_heatbath3d, energy_hist and
    `draws`, the (x, U, W, F, t_new) of every update (F = the number of candidates)."""
    z = q3.clamp(N, placement).copy()
    Q, D, C = len(z), tab.shape[1], N ** 3
    cells = q3._cells(N)
    e_in = q3.energy(N, z)
    E, best, best_sweep, best_state, changed = e_in, e_in, 0, z.copy(), 0
    hist, draws = [e_in], []
    if q3.is_repeated(N, z):
        return {"state": z.astype(np.uint8).reshape(-1), "energy_in": e_in, "energy_out": e_in, "best_energy": e_in, "best_sweep": 0,
                "best_state": z.astype(np.uint8).reshape(-1), "n_changed": 0, "flags": 1,
                "energy_hist": np.full(n_sweeps + 1, e_in, dtype=np.int32), "draws": draws}
    for s in range(n_sweeps):
        g = first_sweep + s
        T = np.array([int(t) for t in tab[s]], dtype=np.uint64)
        for q in range(Q):
            a = q3.counts(N, z, q)  # a(q, t) of every cell, in cell-index order
            idx = cell_index(N, z)
            free = np.ones(C, dtype=bool)
            free[np.delete(idx, q)] = False  # its own cell is a candidate
            a_min = int(a[free].min())
            w = np.where(free, T[np.clip(a - a_min, 0, D - 1)], np.uint64(0))  # (an occupied cell may hold less than a_min: no weight)
            Csum = np.cumsum(w, dtype=np.uint64)
            W = int(Csum[-1])
            x = draw(seed, g * Q + q)
            U = (x * W) >> 64
            p = int(idx[q])
            t = int(np.searchsorted(Csum, np.uint64(U), side="right")) if W else p  # the smallest t with C_t > U
            draws.append((x, U, W, int(free.sum()), t))
            E += int(a[t]) - int(a[p])
            changed += t != p
            z[q] = cells[t]
        hist.append(E)
        if E < best:
            best, best_sweep, best_state = E, s + 1, z.copy()
    return {"state": z.astype(np.uint8).reshape(-1), "energy_in": e_in, "energy_out": E, "best_energy": best, "best_sweep": best_sweep,
            "best_state": best_state.astype(np.uint8).reshape(-1), "n_changed": changed, "flags": 0,
            "energy_hist": np.array(hist, dtype=np.int32), "draws": draws}


def sweeps_many(N, states, seeds, betas, Q=None, first_sweep=0, tab=None):
    Q = N * N if Q is None else Q
    tab = hu.table(betas) if tab is None else tab
    n_sweeps = len(betas) if betas is not None else len(tab)
    rows = [sweeps(N, s, int(seed), tab, n_sweeps, first_sweep) for s, seed in zip(np.asarray(states).reshape(-1, 3 * Q), seeds)]
    return {k: np.stack([np.asarray(r[k]) for r in rows]) for k in FIELDS + ("energy_hist",)}


def assert_equal(got, want, what, hist=False, fields=FIELDS):
    for k in tuple(fields) + (("energy_hist",) if hist else ()):
        g, w = np.asarray(got[k]).astype(np.int64), np.asarray(want[k]).astype(np.int64)
        np.testing.assert_array_equal(g.reshape(w.shape), w, err_msg=f"{what}: {k}")


# ---- the same rule over many chains at once (the stationarity test runs 8 192 chains): NumPy over the chain axis, Python integers for x W

def _philox_many(c0, c1, k0, k1):
    """philox4x32-10 with counter (c0, c1, 0, 0) and key (k0, k1) on uint64 arrays that hold 32-bit words."""
    c0, c1, k0, k1 = (np.asarray(v, dtype=np.uint64) & np.uint64(MASK) for v in (c0, c1, k0, k1))
    c2 = c3 = np.zeros_like(c0)
    m = np.uint64(MASK)
    for _ in range(10):
        p0, p1 = np.uint64(hu.M0) * c0, np.uint64(hu.M1) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & m, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & m
        k0, k1 = (k0 + np.uint64(hu.W0)) & m, (k1 + np.uint64(hu.W1)) & m
    return c0, c1, c2, c3


def sweeps_batch(N, states, seeds, tab, n_sweeps, first_sweep=0):
    """n chains of distinct cells through the rule; returns (state uint8[n][3 Q], energy_out int64[n])."""
    z = np.minimum(np.asarray(states, dtype=np.int64).reshape(len(seeds), -1, 3), N - 1).copy()
    n, Q, D, C = z.shape[0], z.shape[1], tab.shape[1], N ** 3
    cells = q3._cells(N)
    seeds = np.asarray(seeds, dtype=np.uint64)
    rows = np.arange(n)
    for s in range(n_sweeps):
        T = tab[s].astype(np.uint64)
        for q in range(Q):
            d = np.abs(cells[None, :, None, :] - z[:, None, :, :])  # chains x cells x queens x 3
            att = ((d == 0) | (d == d.max(axis=3, keepdims=True))).all(axis=3)
            att[:, :, q] = False
            a = att.sum(axis=2)
            idx = (z[:, :, 0] * N + z[:, :, 1]) * N + z[:, :, 2]
            free = np.ones((n, C), dtype=bool)
            for o in range(Q):
                if o != q:
                    free[rows, idx[:, o]] = False
            a_min = np.where(free, a, 1 << 20).min(axis=1)
            w = np.where(free, T[np.clip(a - a_min[:, None], 0, D - 1)], np.uint64(0))
            Csum = np.cumsum(w, axis=1, dtype=np.uint64)
            u = (first_sweep + s) * Q + q
            r = _philox_many(np.full(n, (u >> 1) & MASK), np.full(n, u >> 33), seeds, np.full(n, 2))
            x = (r[2] | r[3] << np.uint64(32)) if u & 1 else (r[0] | r[1] << np.uint64(32))
            U = np.array([(int(xx) * int(ww)) >> 64 for xx, ww in zip(x, Csum[:, -1])], dtype=np.uint64)
            t = (Csum <= U[:, None]).sum(axis=1)  # the smallest t with C_t > U
            z[:, q] = cells[t]
    E = np.array([q3.energy(N, zz) for zz in z], dtype=np.int64)
    return z.astype(np.uint8).reshape(n, -1), E


@functools.lru_cache(maxsize=None)
def boltzmann_energy_shares(N, Q, beta):
    """P(E) of exp(-beta E) over ALL ordered placements of Q queens on distinct cells of a small cube, as {E: probability}."""
    import itertools

    cells = q3._cells(N)
    att = q3.attack_matrix(cells, cells)
    np.fill_diagonal(att, False)
    perms = np.array(list(itertools.permutations(range(N ** 3), Q)), dtype=np.int64)
    E = np.zeros(len(perms), dtype=np.int64)
    for a in range(Q):
        for b in range(a + 1, Q):
            E += att[perms[:, a], perms[:, b]]
    w = np.exp(-np.float64(beta) * E)
    return len(perms), {int(e): float(w[E == e].sum() / w.sum()) for e in np.unique(E)}


def chi2(energies, shares):
    n = len(energies)
    return float(sum((int((np.asarray(energies) == e).sum()) - n * p) ** 2 / (n * p) for e, p in shares.items()))
