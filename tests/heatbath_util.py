"""The heat-bath rule of include/mcq.h (mcq_heatbath) restated in NumPy and Python integers, from the text of the rule and from nothing
else: its own Philox for general counters and keys, the weight table, and the sweep.  a(c, k) is the quench rule's (items 1 - 2), which
tests/quench_util.py restates and tests/golden/conflicts.npz pins to the reference."""
import numpy as np

from tests import quench_util as qu

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox(ctr, key):
    """philox4x32-10 on Python integers: (4 counter words, 2 key words) -> 4 output words."""
    c0, c1, c2, c3 = (int(x) & MASK for x in ctr)
    k0, k1 = (int(x) & MASK for x in key)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return [c0, c1, c2, c3]


def word(seed, w):
    """Word w (a Python integer below 2^63) of the heat-bath stream of a chain seeded `seed`: key word 1."""
    b = w >> 2
    return philox((b & MASK, b >> 32, 0, 0), (seed, 1))[w & 3]


def table(betas):
    """T[s][d] = floor(2^24 exp(-beta_s d)), one row per sweep; D = 1 + the first d with T = 0 over the rows, at most 512; zero-padded."""
    rows = []
    for beta in betas:
        row = []
        for d in range(512):
            t = int(np.floor(np.float64(2.0**24) * np.exp(np.float64(-beta) * np.float64(d))))
            row.append(t)
            if t == 0:
                break
        rows.append(row)
    if not rows:
        return np.full((1, 1), 1 << 24, dtype=np.uint32)
    D = min(512, max(len(r) for r in rows))
    return np.array([(r + [0] * D)[:D] for r in rows], dtype=np.uint32)


def sweeps(N, board, seed, tab, n_sweeps, first_sweep=0):
    """One chain through the rule with the rows tab[0 .. n_sweeps - 1]; returns a dict with the fields of mcq_heatbath, energy_hist and
    `words`, the (x, U, W) of every update."""
    h = qu.clamp(N, board).copy()
    Q, D = N * N, tab.shape[1]
    e_in = qu.energy(N, h)
    E, best, best_sweep, best_state, changed = e_in, e_in, 0, h.copy(), 0
    hist, words = [e_in], []
    for s in range(n_sweeps):
        g = first_sweep + s
        T = [int(t) for t in tab[s]]
        for c in range(Q):
            a = [int(v) for v in qu.column(N, h, c)]
            a_min = min(a)
            C, tot = [], 0
            for k in range(N):
                tot = (tot + T[min(a[k] - a_min, D - 1)]) & MASK
                C.append(tot)
            W = C[-1]
            x = word(seed, g * Q + c)
            U = (x * W) >> 32
            k_new = next((k for k in range(N) if C[k] > U), N - 1)  # (W = 0, a table with T[0] = 0: no such k, the height N - 1)
            words.append((x, U, W))
            E += a[k_new] - a[int(h[c])]
            changed += k_new != int(h[c])
            h[c] = k_new
        hist.append(E)
        if E < best:
            best, best_sweep, best_state = E, s + 1, h.copy()
    return {"state": h.astype(np.uint8), "energy_in": e_in, "energy_out": E, "best_energy": best, "best_sweep": best_sweep,
            "best_state": best_state.astype(np.uint8), "n_changed": changed, "energy_hist": np.array(hist, dtype=np.int32), "words": words}


FIELDS = ("state", "energy_in", "energy_out", "best_energy", "best_sweep", "best_state", "n_changed")


def sweeps_many(N, states, seeds, betas, first_sweep=0):
    tab = table(betas)
    rows = [sweeps(N, s, int(seed), tab, len(betas), first_sweep) for s, seed in zip(np.asarray(states).reshape(-1, N * N), seeds)]
    return {k: np.stack([np.asarray(r[k]) for r in rows]) for k in FIELDS + ("energy_hist",)}


def assert_equal(got, want, what, hist=False):
    for k in FIELDS + (("energy_hist",) if hist else ()):
        np.testing.assert_array_equal(np.asarray(got[k]).astype(np.int64), np.asarray(want[k]).astype(np.int64), err_msg=f"{what}: {k}")


def all_placements(N):
    """(heights int64[N^(N^2)][N^2], energies int64[N^(N^2)]) of ALL placements of a small board."""
    Q = N * N
    n = N ** Q
    idx = np.arange(n, dtype=np.int64)
    h = np.stack([(idx // N ** c) % N for c in range(Q)], axis=1)  # [n][Q]
    ii, jj = np.divmod(np.arange(Q), N)
    two = np.zeros(n, dtype=np.int64)
    for c in range(Q):
        for c2 in range(Q):
            if c2 == c:
                continue
            di, dj = abs(ii[c2] - ii[c]), abs(jj[c2] - jj[c])
            if di == 0 or dj == 0 or di == dj:
                d = max(di, dj)
                diff = np.abs(h[:, c2] - h[:, c])
                two += (diff == 0) | (diff == d)
    return h, two // 2


def boltzmann_energy_distribution(N, beta):
    """P(E) of the Boltzmann distribution exp(-beta E) over all placements of a small board, as {E: probability}."""
    _, E = all_placements(N)
    w = np.exp(-np.float64(beta) * E)
    Z = w.sum()
    return {int(e): float(w[E == e].sum() / Z) for e in np.unique(E)}
