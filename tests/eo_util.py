"""The extremal-optimisation rule of include/mcq.h (mcq_eo) restated in NumPy, from the text of the rule and from nothing else, as a
brute force: lambda(c) is counted cell by cell over the lines of every column before every iteration (no table is kept), the columns
are put in order by Python's `sorted` over (-lambda, rho, c), the position j is a count over the whole rank table, Philox is written
out here, and every iteration leaves a trace.  What mcq_eo_host is compared with, and where the tests learn which column moved."""
import functools

import numpy as np

FIELDS = ("state", "energy_in", "energy_out", "best_energy", "best_iter", "best_state", "n_moves", "n_uphill", "n_flat", "n_free", "n_idle",
          "energy_hist")
COUNTERS = ("n_moves", "n_uphill", "n_flat", "n_free", "n_idle")
KEY_WORD = 13
MASK = 0xFFFFFFFF


def philox(ctr, key):
    """philox4x32-10 on Python integers: (4 counter words, 2 key words) -> 4 output words."""
    c = [int(x) & MASK for x in ctr]
    k = [int(x) & MASK for x in key]
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & MASK, (p0 >> 32) ^ c[3] ^ k[1], p0 & MASK]
        k = [(k[0] + 0x9E3779B9) & MASK, (k[1] + 0xBB67AE85) & MASK]
    return c


def block(seed, g):
    """(x0, x1, x2, x3) of iteration g of the chain seeded `seed`."""
    return philox((g & MASK, g >> 32, 0, 0), (seed, KEY_WORD))


def clamp(N, board):
    return np.minimum(np.asarray(board, dtype=np.int64).reshape(-1), N - 1)


@functools.lru_cache(maxsize=None)
def _cells(N):
    """Every ordered pair of distinct columns on one row, board column or diagonal, flat: (c, c', d = max(|di|, |dj|))."""
    ii, jj = (x.ravel() for x in np.indices((N, N)))
    di, dj = np.abs(ii[:, None] - ii[None, :]), np.abs(jj[:, None] - jj[None, :])
    on = ((di == 0) | (dj == 0) | (di == dj)) & ((di != 0) | (dj != 0))
    c, c2 = np.nonzero(on)
    return c, c2, np.maximum(di, dj)[on]


def badness(N, h):
    """lambda(c) for every column: the queens of the aligned columns at distance d whose height is h(c), h(c) - d or h(c) + d."""
    c, c2, d = _cells(N)
    diff = np.abs(h[c] - h[c2])
    return np.bincount(c[(diff == 0) | (diff == d)], minlength=N * N)


@functools.lru_cache(maxsize=None)
def _aligned(N, c):
    """The columns on the row, the board column and the two diagonals of column c: [(c', d)]."""
    i, j = divmod(c, N)
    out = []
    for c2 in range(N * N):
        i2, j2 = divmod(c2, N)
        di, dj = abs(i2 - i), abs(j2 - j)
        if c2 != c and (di == 0 or dj == 0 or di == dj):
            out.append((c2, max(di, dj)))
    return out


def attackers(N, h, c, k):
    """a(c, k), cell by cell: one aligned column after the other."""
    return sum(abs(int(h[c2]) - k) in (0, d) for c2, d in _aligned(N, c))


def eo(N, board, seed, n_iters, rank_cdf=(), move="best", first_iter=0, best_floor=None):
    """One chain through the rule; returns a dict with the fields of mcq_eo plus `trace`, one dict per iteration."""
    Q = N * N
    ranks = [int(x) for x in np.asarray(rank_cdf).reshape(-1)]
    assert 0 <= len(ranks) <= Q - 1 and move in ("best", "random")
    h = clamp(N, board).copy()
    lam = badness(N, h)
    e_in = int(lam.sum()) // 2
    E = e_in
    B = e_in if best_floor is None else min(int(best_floor), e_in)
    best, best_iter = h.copy(), 0
    hist, trace = [E], []
    n = dict.fromkeys(COUNTERS, 0)
    for t in range(n_iters):
        g = first_iter + t
        if E == 0:
            n["n_idle"] += 1
            hist.append(E)
            trace.append({"moved": False, "g": g})
            continue
        x0, x1, x2, x3 = block(seed, g)
        o, oh = (x1 * Q) >> 32, (x2 * N) >> 32
        j = sum(1 for r in ranks if r <= x0)
        lam = badness(N, h)
        assert int(lam.sum()) == 2 * E and int(lam.max()) <= 4 * (N - 1)
        order = sorted(range(Q), key=lambda c: (-int(lam[c]), (c - o) % Q, c))
        c = order[j]
        hc, lc = int(h[c]), int(lam[c])
        assert attackers(N, h, c, hc) == lc
        if move == "best":
            k = min((k for k in range(N) if k != hc), key=lambda k: (attackers(N, h, c, k), (k - oh) % N))
        else:
            k = (x3 * (N - 1)) >> 32
            k += k >= hc
        delta = attackers(N, h, c, k) - lc
        first_of, last_of = j == 0 or lam[order[j - 1]] != lc, j == Q - 1 or lam[order[j + 1]] != lc
        trace.append({"moved": True, "g": g, "c": c, "k": k, "j": j, "o": o, "lam": lc, "delta": delta, "first_of_class": bool(first_of),
                      "last_of_class": bool(last_of), "wrapped": c < o, "class_wraps": bool(((lam == lc) & (np.arange(Q) < o)).any() and ((lam == lc) & (np.arange(Q) >= o)).any()),
                      "class_size": int((lam == lc).sum())})
        n["n_moves"] += 1
        n["n_uphill"] += delta > 0
        n["n_flat"] += delta == 0
        n["n_free"] += lc == 0
        h[c] = k
        E += delta
        if E < B:
            B, best_iter, best = E, t + 1, h.copy()
        hist.append(E)
    out = {"state": h.astype(np.uint8), "energy_in": e_in, "energy_out": E, "best_energy": B, "best_iter": best_iter, "best_state": best.astype(np.uint8),
           "energy_hist": np.array(hist, dtype=np.int64), "trace": trace}
    out.update({k: int(v) for k, v in n.items()})
    return out


def eo_many(N, states, seeds, n_iters, best_floor=None, **kw):
    states = np.asarray(states).reshape(-1, N * N)
    rows = [eo(N, s, int(seed), n_iters, best_floor=None if best_floor is None else best_floor[r], **kw) for r, (s, seed) in enumerate(zip(states, seeds))]
    out = {k: np.stack([np.asarray(r[k]) for r in rows]) for k in FIELDS}
    out["trace"] = [r["trace"] for r in rows]
    return out


def assert_equal(got, want, what, fields=FIELDS):
    for k in fields:
        np.testing.assert_array_equal(np.asarray(got[k]).astype(np.int64), np.asarray(want[k]).astype(np.int64), err_msg=f"{what}: {k}")


def merge(parts):
    """The figures of a run cut into calls, as consequence (b) of the rule combines them."""
    out = {k: sum(p[k] for p in parts) for k in COUNTERS}
    last = parts[-1]
    for k in ("state", "energy_out", "best_energy"):
        out[k] = last[k]
    out["energy_in"] = parts[0]["energy_in"]
    out["energy_hist"] = np.concatenate([parts[0]["energy_hist"]] + [p["energy_hist"][:, 1:] for p in parts[1:]], axis=1)
    out["best_iter"], out["best_state"] = parts[0]["best_iter"].copy(), parts[0]["best_state"].copy()
    done = 0
    for p in parts:
        m = p["best_iter"] > 0
        out["best_iter"][m] = p["best_iter"][m] + done
        out["best_state"][m] = p["best_state"][m]
        done += p["energy_hist"].shape[1] - 1
    return out


def run_cut(fn, N, s, seeds, cuts, first_iter=0, best_floor=None, **kw):
    """fn (eo_states_host, eo_states, eo_many) over the pieces `cuts`, each fed the state and the best_energy of the one before."""
    parts, state, bf, done = [], s, best_floor, first_iter
    for iters in cuts:
        parts.append(fn(N, state, seeds, iters, first_iter=done, best_floor=bf, hist=True, **kw) if fn is not eo_many
                     else fn(N, state, seeds, iters, first_iter=done, best_floor=bf, **kw))
        state, bf, done = parts[-1]["state"], parts[-1]["best_energy"], done + iters
    return parts


def random_boards(N, n, seed, over=False):
    """n random boards of edge N as uint8[n][N*N]; over=True mixes in bytes >= N (the library clamps them)."""
    rs = np.random.RandomState(seed)
    s = rs.randint(0, N, size=(n, N * N)).astype(np.uint8)
    if over:
        s[rs.rand(n, N * N) < 0.05] = 255
    return s


def klarner(N):
    """(3 i + 5 j) mod N: a zero-energy board where gcd(N, 210) = 1."""
    i, j = np.indices((N, N))
    return ((3 * i + 5 * j) % N).astype(np.uint8).reshape(-1)


def step_table(N, j):
    """A rank table that gives position j in every iteration, whatever x0 is: j entries of 0, each of them <= x0."""
    return np.zeros(j, dtype=np.uint32)
