"""The full_3d relinking rule of include/mcq.h (mcq_relink3d) restated in NumPy, from the text of the rule and from nothing else: a brute
force over ALL pairs (moving queen, open target) with an attack matrix of cells x queens (the predicate and the Philox of
tests/tabu3d_util.py, which are NumPy's own and share nothing with the library), E recounted after every step, every placement of the
walk kept and P* picked from the list afterwards, a local search of its own up to N = 5 (quench_queens_host beyond, where a pass over
the cube in NumPy per queen is too slow), and a trace per step.  No attack field, no lists, no packed key: what mcq_relink3d_host and
the kernel are compared with, so that neither is tested against its own idea."""
import numpy as np

from tests import tabu3d_util as t3

FIELDS = ("state", "path_best_state", "distance_in", "n_steps", "path_best_step", "energy_in", "path_best_energy", "path_max_energy",
          "energy_out", "n_moves", "n_passes", "energy_hist", "flags")
KEY_WORD = 10
MASK = 0xFFFFFFFF
OWN_L_MAX_N = 5


def draw(seed, t, walk, N, Q):
    """(o_q, o_t) of step t of walk `walk`."""
    x = t3.philox((t & MASK, walk & MASK, (walk >> 32) & MASK, 0), (int(seed), KEY_WORD))
    return (x[0] * Q) >> 32, (x[1] * N ** 3) >> 32


def _energy(att, idx):
    return int(att[idx].sum() - len(idx)) // 2


def descend(N, z):
    """L on the triples z (int64[Q][3], no two alike): passes of the mcq_quench3d rule until one moves nothing.  Returns (z, moves, passes)."""
    z = z.copy()
    Q, C = len(z), N ** 3
    cells = t3._cells(N)
    idx = t3.index_of(N, z)
    att = t3.attack_matrix(N, z)
    moves = passes = 0
    while True:
        moved = 0
        for q in range(Q):
            a = att.sum(axis=1, dtype=np.int64) - att[:, q]  # a(q, t) for every cell
            now = int(a[idx[q]])
            if now == 0:
                continue
            held = np.zeros(C, dtype=bool)
            held[np.delete(idx, q)] = True
            a = np.where(held, 1 << 30, a)
            t = int(np.argmin(a))  # the smallest cell index of the smallest count
            if a[t] < now:
                z[q], idx[q] = cells[t], t
                att[:, q] = t3.attack_matrix(N, z[q:q + 1])[:, 0]
                moved += 1
        passes += 1
        moves += moved
        if not moved:
            return z, moves, passes


def _local_search(N, z):
    if N <= OWN_L_MAX_N:
        return descend(N, z)
    import mcq_amd

    r = mcq_amd.quench.quench_queens_host(N, z.astype(np.uint8).reshape(1, -1), Q=len(z), conflicts=False)
    return r["state"].reshape(-1, 3).astype(np.int64), int(r["n_moves"][0]), int(r["n_passes"][0])


def relink(N, placement, guide, seed, max_steps=0, min_dist=1, walk=0):
    """One chain through the rule; returns a dict with the fields of mcq_relink3d plus `trace`, one dict per step, and `path`, the cell
    indices of every placement of the walk."""
    z, g = t3.clamp(N, placement).copy(), t3.clamp(N, guide)
    Q, C = len(z), N ** 3
    W = max_steps if max_steps else Q
    cells = t3._cells(N)
    idx = t3.index_of(N, z)
    gset = set(int(c) for c in t3.index_of(N, g))
    att = t3.attack_matrix(N, z)
    e_in = _energy(att, idx)
    flags = (1 if len(set(idx.tolist())) < Q else 0) | (2 if len(gset) < Q else 0)
    flat = z.astype(np.uint8).reshape(-1)
    if flags:  # item 6
        return {"state": flat, "path_best_state": flat, "distance_in": 0, "n_steps": 0, "path_best_step": 0, "energy_in": e_in, "path_best_energy": e_in,
                "path_max_energy": e_in, "energy_out": e_in, "n_moves": 0, "n_passes": 0, "energy_hist": np.full(W + 1, e_in, dtype=np.int64),
                "flags": flags, "trace": [], "path": [idx.copy()]}
    d0 = len(gset - set(idx.tolist()))
    assert d0 == sum(int(c) not in gset for c in idx)
    n_steps = d0 if max_steps == 0 else min(d0, max_steps)
    E, hist, path, trace = e_in, [e_in], [idx.copy()], []
    for t in range(n_steps):
        oq, ot = draw(seed, t, walk, N, Q)
        M = np.array([q for q in range(Q) if int(idx[q]) not in gset], dtype=np.int64)
        T = np.array(sorted(gset - set(idx.tolist())), dtype=np.int64)
        S = np.count_nonzero(att, axis=1).astype(np.int64)  # the queens that hold or attack each cell
        delta = S[T][None, :] - att[np.ix_(T, M)].T.astype(np.int64) - (S[idx[M]] - 1)[:, None]  # [M][T]
        d = int(delta.min())
        mi, ti = np.nonzero(delta == d)
        w = np.lexsort(((T[ti] - ot) % C, (M[mi] - oq) % Q))[0]  # (the last key is the first to count)
        q, c = int(M[mi[w]]), int(T[ti[w]])
        trace.append({"delta": d, "ties": len(mi), "q": q, "c": c, "rho_q": (q - oq) % Q, "rho_t": (c - ot) % C, "wrapped_q": q < oq, "wrapped_t": c < ot,
                      "on_line": bool(att[c, q]), "m": len(M), "oq": oq, "ot": ot})
        z[q], idx[q] = cells[c], c
        att[:, q] = t3.attack_matrix(N, z[q:q + 1])[:, 0]
        E += d
        assert E == _energy(att, idx), "E tracked through delta is the recount"
        hist.append(E)
        path.append(idx.copy())
    if max_steps == 0:
        assert set(idx.tolist()) == gset
    cand = [t for t in range(1, n_steps + 1) if t >= max(1, min_dist) and d0 - t >= min_dist]
    best_step = min(cand, key=lambda t: (hist[t], t)) if cand else 0
    pstar = cells[path[best_step]]
    out_z, moves, passes = _local_search(N, pstar)
    e_out = _energy(t3.attack_matrix(N, out_z), t3.index_of(N, out_z))
    return {"state": out_z.astype(np.uint8).reshape(-1), "path_best_state": pstar.astype(np.uint8).reshape(-1), "distance_in": d0, "n_steps": n_steps,
            "path_best_step": best_step, "energy_in": e_in, "path_best_energy": hist[best_step], "path_max_energy": max(hist), "energy_out": e_out,
            "n_moves": moves, "n_passes": passes, "energy_hist": np.array(hist + [hist[-1]] * (W - n_steps), dtype=np.int64), "flags": 0,
            "trace": trace, "path": path}


def relink_many(N, states, guides, seeds, Q=None, rows=None, **kw):
    Q = N * N if Q is None else Q
    states, guides = np.asarray(states).reshape(-1, 3 * Q), np.asarray(guides).reshape(-1, 3 * Q)
    pick = range(len(states))[rows] if rows is not None else range(len(states))
    res = [relink(N, states[r], guides[r], int(seeds[r]), **kw) for r in pick]
    out = {k: np.stack([np.asarray(r[k]) for r in res]) for k in FIELDS}
    out["trace"] = [r["trace"] for r in res]
    return out


def assert_equal(got, want, what, rows=None, fields=FIELDS):
    for k in fields:
        g, w = np.asarray(got[k]).astype(np.int64), np.asarray(want[k]).astype(np.int64)
        if rows is not None:
            g = g[rows]
        np.testing.assert_array_equal(g.reshape(w.shape), w, err_msg=f"{what}: {k}")


def tally(traces, host, minima=False):
    """What compared calls hold, from the restatement's traces and the host code's outputs (rows alike).  minima: both endpoints are
    local minima, so a result below both is a gain of the relinking and not of the descent alone."""
    n = dict.fromkeys(("steps", "ties", "wrapped_q", "wrapped_t", "rises", "falls", "on_line", "off_line"), 0)
    for chain in traces:
        for tr in chain:
            n["steps"] += 1
            n["ties"] += tr["ties"] >= 2
            n["wrapped_q"] += tr["wrapped_q"]
            n["wrapped_t"] += tr["wrapped_t"]
            n["rises"] += tr["delta"] > 0
            n["falls"] += tr["delta"] < 0
            n["on_line"] += tr["on_line"]
            n["off_line"] += not tr["on_line"]
    h = {k: np.asarray(v).astype(np.int64) for k, v in host.items() if k != "trace"}
    d0, step, md_last = h["distance_in"], h["path_best_step"], h.get("last_candidate")
    n["pstar_inside"] = int(((step > 0) & (step < md_last)).sum()) if md_last is not None else 0
    n["pstar_last"] = int(((step > 0) & (step == md_last)).sum()) if md_last is not None else 0
    n["pstar_absent"] = int(((step == 0) & (h["flags"] == 0)).sum())
    n["l_moves"] = int((h["n_moves"] > 0).sum())
    n["l_still"] = int(((h["n_moves"] == 0) & (h["flags"] == 0)).sum())
    whole = (h["n_steps"] == d0) & (h["flags"] == 0)  # the walks that end on the guide: entry d0 of the history is its energy
    guide_e = h["energy_hist"][np.arange(len(d0)), np.where(whole, d0, 0)]
    n["below_both"] = int((whole & (d0 > 0) & (h["energy_out"] < np.minimum(h["energy_in"], guide_e))).sum()) if minima else 0
    return n
