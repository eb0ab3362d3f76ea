"""The extremal-optimisation rule of include/mcq.h for full_3d placements (mcq_eo3d) restated in NumPy, from the text of the rule and
from nothing else, as a brute force: lambda(q) and a(q, t) are pairwise attack tests over the queens (no field is kept), the queens are
put in order by Python's `sorted` over (-lambda, rho_q, q), the position j is a count over the whole rank table, both moves walk the
free cells in the order of their index, Philox is written out here on Python integers, and every iteration leaves a trace.  What
mcq_eo3d_host is compared with, and where the tests learn which queen moved and where it went."""
import numpy as np

FIELDS = ("state", "energy_in", "energy_out", "best_energy", "best_iter", "best_state", "n_moves", "n_uphill", "n_flat", "n_free", "n_idle",
          "energy_hist", "flags")
COUNTERS = ("n_moves", "n_uphill", "n_flat", "n_free", "n_idle")
KEY_WORD = 14
MASK = 0xFFFFFFFF
REPEATED = 1


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


def clamp(N, placement):
    """The triples of a placement as int16[Q][3], every byte clamped to N - 1."""
    return np.minimum(np.asarray(placement, dtype=np.int16).reshape(-1, 3), N - 1)


def cells_of(N, pos):
    p = pos.astype(np.int64)
    return (p[:, 0] * N + p[:, 1]) * N + p[:, 2]


def triples_of(N, cells):
    c = np.asarray(cells, dtype=np.int64)
    return np.stack([c // (N * N), (c // N) % N, c % N], axis=-1).astype(np.int16)


def attackers(queens, targets, chunk=2048):
    """For every target triple, the number of the queens that hold or attack it: the non-zero ones among |di|, |dj|, |dk| all equal."""
    queens, targets = np.asarray(queens, dtype=np.int8).reshape(-1, 3), np.asarray(targets, dtype=np.int8).reshape(-1, 3)  # (coordinates < 32)
    out = np.zeros(len(targets), dtype=np.int64)
    for a in range(0, len(targets), chunk):
        di, dj, dk = (np.abs(targets[a:a + chunk, None, x] - queens[None, :, x]) for x in range(3))
        m = np.maximum(di, np.maximum(dj, dk))
        out[a:a + chunk] = (((di == 0) | (di == m)) & ((dj == 0) | (dj == m)) & ((dk == 0) | (dk == m))).sum(axis=1)
    return out


def badness(pos):
    """lambda(q) for every queen: the OTHER queens that attack it (a queen in the same cell among them)."""
    return attackers(pos, pos) - 1


def eo3d(N, placement, seed, n_iters, rank_cdf=(), move="best", first_iter=0, best_floor=None):
    """One chain through the rule; returns a dict with the fields of mcq_eo3d plus `trace`, one dict per iteration."""
    pos = clamp(N, placement).copy()
    Q, C = len(pos), N ** 3
    ranks = [int(x) for x in np.asarray(rank_cdf).reshape(-1)]
    assert 2 <= Q <= C - 1 and 0 <= len(ranks) <= Q - 1 and move in ("best", "random")
    lam = badness(pos)
    e_in = int(lam.sum()) // 2
    n = dict.fromkeys(COUNTERS, 0)
    if len(set(cells_of(N, pos).tolist())) < Q:  # REPEATED: handed back unmoved
        out = {"state": pos.astype(np.uint8).reshape(-1), "energy_in": e_in, "energy_out": e_in, "best_energy": e_in, "best_iter": 0,
               "best_state": pos.astype(np.uint8).reshape(-1), "energy_hist": np.full(n_iters + 1, e_in, dtype=np.int64), "flags": REPEATED, "trace": []}
        out.update(n)
        return out
    E = e_in
    B = e_in if best_floor is None else min(int(best_floor), e_in)
    best, best_iter = pos.copy(), 0
    hist, trace = [E], []
    F = C - Q
    for t in range(n_iters):
        g = first_iter + t
        if E == 0:
            n["n_idle"] += 1
            hist.append(E)
            trace.append({"moved": False, "g": g})
            continue
        x0, x1, x2, x3 = block(seed, g)
        oq, ot = (x1 * Q) >> 32, (x2 * C) >> 32
        j = sum(1 for r in ranks if r <= x0)
        lam = badness(pos)
        assert int(lam.sum()) == 2 * E and int(lam.max()) <= 13 * (N - 1)
        order = sorted(range(Q), key=lambda q: (-int(lam[q]), (q - oq) % Q, q))
        q = order[j]
        lq = int(lam[q])
        held = set(cells_of(N, pos).tolist())
        free = [c for c in range(C) if c not in held]  # the walk over the free cells, in the order of their index
        assert len(free) == F
        others = np.delete(pos, q, axis=0)
        if move == "best":
            a = attackers(others, triples_of(N, free))
            m = min(range(F), key=lambda i: (int(a[i]), (free[i] - ot) % C))
            at = int(a[m])
        else:
            m = (x3 * F) >> 32
            at = int(attackers(others, triples_of(N, free[m:m + 1]))[0])
        cell = free[m]
        delta = at - lq
        members = lam == lq
        trace.append({"moved": True, "g": g, "q": q, "j": j, "oq": oq, "ot": ot, "lam": lq, "class_size": int(members.sum()),
                      "class_wraps": bool((members & (np.arange(Q) < oq)).any() and (members & (np.arange(Q) >= oq)).any()),
                      "first_of_class": bool(j == 0 or lam[order[j - 1]] != lq), "last_of_class": bool(j == Q - 1 or lam[order[j + 1]] != lq),
                      "wrapped": q < oq, "t": cell, "m": m, "F": F, "delta": delta, "t_wrapped": cell < ot})
        n["n_moves"] += 1
        n["n_uphill"] += delta > 0
        n["n_flat"] += delta == 0
        n["n_free"] += lq == 0
        pos[q] = triples_of(N, [cell])[0]
        E += delta
        if E < B:
            B, best_iter, best = E, t + 1, pos.copy()
        hist.append(E)
    out = {"state": pos.astype(np.uint8).reshape(-1), "energy_in": e_in, "energy_out": E, "best_energy": B, "best_iter": best_iter,
           "best_state": best.astype(np.uint8).reshape(-1), "energy_hist": np.array(hist, dtype=np.int64), "flags": 0, "trace": trace}
    out.update({k: int(v) for k, v in n.items()})
    return out


def eo3d_many(N, states, seeds, n_iters, Q=None, best_floor=None, **kw):
    Q = N * N if Q is None else Q
    states = np.asarray(states).reshape(-1, 3 * Q)
    rows = [eo3d(N, s, int(seed), n_iters, best_floor=None if best_floor is None else best_floor[r], **kw) for r, (s, seed) in enumerate(zip(states, seeds))]
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
    for k in ("state", "energy_out", "best_energy", "flags"):
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
    """fn (eo_queens_host, eo_queens, eo3d_many) over the pieces `cuts`, each fed the state and the best_energy of the one before."""
    parts, state, bf, done = [], s, best_floor, first_iter
    for iters in cuts:
        parts.append(fn(N, state, seeds, iters, first_iter=done, best_floor=bf, hist=True, **kw) if fn is not eo3d_many
                     else fn(N, state, seeds, iters, first_iter=done, best_floor=bf, **kw))
        state, bf, done = parts[-1]["state"], parts[-1]["best_energy"], done + iters
    return parts


def random_queens(N, Q, n, seed, over=False):
    """n random placements of Q queens in distinct cells of the cube of edge N as uint8[n][3 Q]; over=True turns some bytes N - 1 into
    bytes >= N (the library clamps them back, so the cells stay distinct)."""
    rs = np.random.RandomState(seed)
    out = np.empty((n, Q, 3), dtype=np.uint8)
    for r in range(n):
        out[r] = triples_of(N, rs.permutation(N ** 3)[:Q]).astype(np.uint8)
    if over:
        top = out == N - 1
        hit = top & (rs.rand(n, Q, 3) < 0.3)
        if top.any() and not hit.any():
            hit.reshape(-1)[np.flatnonzero(top)[0]] = True
        out[hit] = rs.randint(N, 256, size=int(hit.sum())).astype(np.uint8)
    return out.reshape(n, 3 * Q)


def cube_without(N, holes):
    """The placement that fills the cube of edge N except the cells `holes`, in the order of the cell index: uint8[3 (N^3 - len(holes))]."""
    keep = np.setdiff1d(np.arange(N ** 3), np.asarray(holes))
    return triples_of(N, keep).astype(np.uint8).reshape(-1)


def calm_queens(N, Q, seed):
    """Q queens of which none attacks another, taken greedily from a random order of the cells: uint8[3 Q], a placement of energy 0."""
    rs = np.random.RandomState(seed)
    kept = np.zeros((0, 3), dtype=np.int16)
    for cell in rs.permutation(N ** 3):
        t = triples_of(N, [cell])
        if not attackers(kept, t)[0]:
            kept = np.concatenate([kept, t])
        if len(kept) == Q:
            return kept.astype(np.uint8).reshape(-1)
    raise ValueError(f"no {Q} calm queens found at N = {N}")


def step_table(j):
    """A rank table that gives position j in every iteration, whatever x0 is: j entries of 0, each of them <= x0."""
    return np.zeros(j, dtype=np.uint32)
