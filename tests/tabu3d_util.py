"""The full_3d tabu rule of include/mcq.h (mcq_tabu3d) restated in NumPy, from the text of the rule and from nothing else: a brute force
over ALL pairs (conflicting queen, free cell) with an attack matrix of cells x queens recounted before every iteration, its own attack
predicate, its own Philox, absolute stamps in an int64 array, and a trace per iteration.  No attack field, no pass over the cube apart
from the pass over a queen's lines: what mcq_tabu3d_host and the kernel are compared with, so that neither is tested against its own
idea.  Below the rule: the inputs that sleep until iteration 2^15 of a call with the window that restates them, and the placements at
the ends of the kernel's packed key."""
import functools

import numpy as np

FIELDS = ("state", "energy_in", "energy_out", "best_energy", "best_iter", "best_state", "n_moves", "n_aspired", "n_uphill", "n_stalled",
          "energy_hist", "tabu_out", "flags")
COUNTERS = ("n_moves", "n_aspired", "n_uphill", "n_stalled")
KEY_WORD = 8
SPAN = (1 << 14) - 1
REBASE = 1 << 15
MASK = 0xFFFFFFFF
LONGEST = dict(tenure=8192, tenure_rand=4095, tenure_conf=64)


def philox(ctr, key):
    """philox4x32-10 on Python integers."""
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & MASK, p1 & MASK, ((p0 >> 32) ^ c3 ^ k1) & MASK, p0 & MASK
        k0, k1 = (k0 + 0x9E3779B9) & MASK, (k1 + 0xBB67AE85) & MASK
    return c0, c1, c2, c3


def draw(seed, g, N, Q, tenure_rand):
    """(o_q, jitter, o_t) of iteration g."""
    x = philox((g & MASK, g >> 32, 0, 0), (int(seed), KEY_WORD))
    return (x[0] * Q) >> 32, (x[1] * (tenure_rand + 1)) >> 32, (x[2] * N ** 3) >> 32


@functools.lru_cache(maxsize=None)
def _cells(N):
    return np.stack(np.unravel_index(np.arange(N ** 3), (N, N, N)), axis=1).astype(np.int64)


def attack_matrix(N, z):
    """bool[N^3][Q]: cell t is queen q's cell or on one of the 13 lines through it: of the coordinate differences, those that are not 0
    are all the same in size.  (Axis by axis in int16: a dense cube at N = 17 is 22 M pairs.)"""
    cells = _cells(N).astype(np.int16)
    z = np.asarray(z).astype(np.int16)
    d = [np.abs(cells[:, None, x] - z[None, :, x]) for x in range(3)]
    m = np.maximum(np.maximum(d[0], d[1]), d[2])
    ok = np.ones(m.shape, dtype=bool)
    for x in range(3):
        ok &= (d[x] == 0) | (d[x] == m)
    return ok


def clamp(N, placement):
    return np.minimum(np.asarray(placement, dtype=np.int64).reshape(-1, 3), N - 1)


def index_of(N, z):
    return (z[:, 0] * N + z[:, 1]) * N + z[:, 2]


def energy(N, placement):
    z = clamp(N, placement)
    return int(attack_matrix(N, z)[index_of(N, z)].sum() - len(z)) // 2


def tabu(N, placement, seed, n_iters, tenure=10, tenure_rand=0, tenure_conf=0, first_iter=0, tabu_in=None, best_floor=None):
    """One chain through the rule; returns a dict with the fields of mcq_tabu3d plus `trace`, one dict per iteration."""
    z = clamp(N, placement).copy()
    Q, C = len(z), N ** 3
    cells = _cells(N)
    idx = index_of(N, z)
    att = attack_matrix(N, z)
    e_in = int(att[idx].sum() - Q) // 2
    stamps_in = np.zeros(C, dtype=np.int64) if tabu_in is None else np.asarray(tabu_in, dtype=np.int64).reshape(C)
    out = {"state": z.astype(np.uint8).reshape(-1), "best_state": z.astype(np.uint8).reshape(-1), "energy_in": e_in, "energy_out": e_in,
           "best_iter": 0, "flags": 0, "trace": []}
    out.update(dict.fromkeys(COUNTERS, 0))
    if len(np.unique(idx)) < Q:  # item 7
        out.update(best_energy=e_in, flags=1, energy_hist=np.full(n_iters + 1, e_in, dtype=np.int64), tabu_out=stamps_in.copy())
        return out
    T = first_iter + stamps_in
    E = e_in
    B = e_in if best_floor is None else min(int(best_floor), e_in)
    best, best_iter = z.copy(), 0
    hist, trace = [E], []
    n = dict.fromkeys(COUNTERS, 0)
    qs = np.arange(Q)
    for t in range(n_iters):
        g = first_iter + t
        oq, jitter, ot = draw(seed, g, N, Q, tenure_rand)
        total = att.sum(axis=1, dtype=np.int32)
        a = total[:, None] - att  # a(q, t) for every cell and queen: the others that hold or attack t
        now = a[idx, qs]
        assert int(now.sum()) == 2 * E
        free = np.ones(C, dtype=bool)
        free[idx] = False
        delta = a - now[None, :]
        cand = free[:, None] & (now[None, :] > 0)
        is_tabu = (T > g)[:, None]
        adm = cand & (~is_tabu | (E + delta < B))
        F = int((now > 0).sum())
        tr = {"F": F, "E": E, "g": g, "moved": False, "candidates": int(cand.sum())}
        if not adm.any():
            n["n_stalled"] += 1
        else:
            d = int(delta[adm].min())
            ct, cq = np.nonzero(adm & (delta == d))  # the ties of the smallest delta: the smallest rho_q, then the smallest rho_t
            w = np.lexsort(((ct - ot) % C, (cq - oq) % Q))[0]  # (the last key is the first to count)
            tc, q = int(ct[w]), int(cq[w])
            L = min(SPAN, tenure + jitter + (tenure_conf * F) // 16)
            tabu_move = bool(T[tc] > g)
            tr.update(moved=True, tabu=tabu_move, delta=d, L=L, q=q, t=tc, new_best=E + d < B, on_line=bool(att[tc, q]),
                      wrapped_q=q < oq, wrapped_t=tc < ot, ties=len(ct))
            n["n_moves"] += 1
            n["n_aspired"] += int(tabu_move)
            n["n_uphill"] += int(d > 0)
            T[idx[q]] = g + 1 + L
            z[q] = cells[tc]
            idx[q] = tc
            att[:, q] = attack_matrix(N, z[q:q + 1])[:, 0]
            E += d
            if E < B:
                B, best_iter, best = E, t + 1, z.copy()
        hist.append(E)
        trace.append(tr)
    out.update(state=z.astype(np.uint8).reshape(-1), energy_out=E, best_energy=B, best_iter=best_iter, best_state=best.astype(np.uint8).reshape(-1),
               energy_hist=np.array(hist, dtype=np.int64), tabu_out=np.maximum(0, T - (first_iter + n_iters)), trace=trace)
    out.update(n)
    assert out["tabu_out"].max() < 1 << 16
    return out


def tabu_many(N, states, seeds, n_iters, Q=None, tabu_in=None, best_floor=None, **kw):
    Q = N * N if Q is None else Q
    states = np.asarray(states).reshape(-1, 3 * Q)
    rows = [tabu(N, s, int(seed), n_iters, tabu_in=None if tabu_in is None else np.asarray(tabu_in).reshape(len(states), -1)[r],
                 best_floor=None if best_floor is None else best_floor[r], **kw) for r, (s, seed) in enumerate(zip(states, seeds))]
    out = {k: np.stack([np.asarray(r[k]) for r in rows]) for k in FIELDS}
    out["trace"] = [r["trace"] for r in rows]
    return out


def assert_equal(got, want, what, fields=FIELDS):
    for k in fields:
        g, w = np.asarray(got[k]).astype(np.int64), np.asarray(want[k]).astype(np.int64)
        np.testing.assert_array_equal(g.reshape(w.shape), w, err_msg=f"{what}: {k}")


def row(res, r):
    return {k: np.asarray(v)[r] for k, v in res.items() if k != "trace"}


def merge(parts):
    """The figures of a run cut into calls, as consequence (b) of the rule combines them."""
    out = {k: sum(p[k] for p in parts) for k in COUNTERS}
    last = parts[-1]
    for k in ("state", "energy_out", "best_energy", "tabu_out", "flags"):
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


def run_cut(fn, N, s, seeds, cuts, first_iter=0, tabu_in=None, best_floor=None, **kw):
    """fn (tabu_queens_host, tabu_queens, tabu_many) over the pieces `cuts`, each fed the state, tabu_out and best_energy of the one before."""
    parts, state, ti, bf, done = [], s, tabu_in, best_floor, first_iter
    for iters in cuts:
        parts.append(fn(N, state, seeds, iters, first_iter=done, tabu_in=ti, best_floor=bf, **kw))
        state, ti, bf, done = parts[-1]["state"], parts[-1]["tabu_out"], parts[-1]["best_energy"], done + iters
    return parts


def tally(traces):
    """What the traces of compared runs hold: moves, uphill moves, aspired moves, stalls (all, and above E = 0), winners on the moved
    queen's own lines, and winners in front of either offset."""
    n = dict.fromkeys(("moves", "uphill", "aspired", "stalls", "stall_above_0", "on_line", "wrapped_q", "wrapped_t"), 0)
    for chain in traces:
        for tr in chain:
            if not tr["moved"]:
                n["stalls"] += 1
                n["stall_above_0"] += tr["E"] > 0
                continue
            n["moves"] += 1
            n["uphill"] += tr["delta"] > 0
            n["aspired"] += tr["tabu"]
            n["on_line"] += tr["on_line"]
            n["wrapped_q"] += tr["wrapped_q"]
            n["wrapped_t"] += tr["wrapped_t"]
    return n


# Inputs that sleep, then wake across the move of the kernel's stamp base.  With every free cell of a chain tabu and best_floor = 0 the
# rule admits nothing: the chain stalls, and its placement and absolute stamps stay as they are until the first stamp expires.  So the
# run from iteration W on is, by consequence (b), the run with first_iter = W, tabu_in - W and best_floor = 0, and only that window
# has to be restated, while a kernel has to run all of it in one call and move its base at iteration REBASE of the call.
def sleeping(N, n, seed, lo, hi):
    """tabu_in of n chains whose every cell is tabu until it expires at an iteration of [lo, hi) of the call."""
    return np.random.RandomState(seed).randint(lo, hi, size=(n, N ** 3)).astype(np.uint16)


def wake(N, states, seeds, n_iters, tabu_in, W, Q=None, **kw):
    """The outputs of the sleeping run of n_iters >= W iterations from iteration 0, restated over [W, n_iters) alone."""
    n = len(states)
    win = tabu_many(N, states, seeds, n_iters - W, Q=Q, first_iter=W, tabu_in=np.asarray(tabu_in).astype(np.int64) - W, best_floor=np.zeros(n, dtype=np.int64), **kw)
    out = dict(win)
    out["n_stalled"] = win["n_stalled"] + W
    out["best_iter"] = np.where(win["best_iter"] > 0, win["best_iter"] + W, 0)
    out["energy_hist"] = np.concatenate([np.repeat(win["energy_hist"][:, :1], W, axis=1), win["energy_hist"]], axis=1)
    return out


def assert_asleep(got, W, what):
    """The premise of `wake`, on the outputs of code that ran the whole call: nothing moved before iteration W."""
    hist = np.asarray(got["energy_hist"]).astype(np.int64)
    assert (hist[:, : W + 1] == hist[:, :1]).all() and (np.asarray(got["n_stalled"]) >= W).all(), f"{what}: a chain moved before iteration {W}"
    assert (np.asarray(got["n_moves"]) + np.asarray(got["n_stalled"]) == hist.shape[1] - 1).all(), what


# Placements at the ends of the kernel's packed key (delta + 403) << 30 | rho_q << 15 | rho_t.  How they were derived is in DESIGN.md.
def _cell(N, i, j, k):
    return (i * N + j) * N + k


def star(N, centre=None):
    """The centre cell and every cell on the 13 lines through it, as cell indices, the centre first."""
    c = (N // 2,) * 3 if centre is None else centre
    z = np.array([c], dtype=np.int64)
    on = np.flatnonzero(attack_matrix(N, z)[:, 0])
    ci = _cell(N, *c)
    return [ci] + [int(x) for x in on if x != ci]


def placement_of(N, cells):
    cells = np.asarray(cells, dtype=np.int64)
    return np.stack([cells // (N * N), (cells // N) % N, cells % N], axis=1).astype(np.uint8).reshape(1, -1)


KEY_N = (19, 32)
KEY_RISE = {19: 192, 32: 342}  # the smallest delta onto the centre: what the restatement takes there (queens with delta up to 13 (N - 1) - 1 and 396 lose)
ONE_SEED = np.array([12345], dtype=np.uint32)


@functools.lru_cache(maxsize=None)
def key_case(N, kind):
    """(placement, seeds, iterations, keywords, the restatement's result) at an end of delta.  "fall": every cell of the star holds a
    queen, so the centre queen is attacked along all its lines and leaves for a cell that nothing attacks.  "rise": the star without its
    centre and a pair of queens off its lines; every cell is tabu for 50 iterations but the centre, under best_floor = 0, so each
    conflicting queen's one admissible move is onto the centre, where every other queen of the star attacks it."""
    st = star(N)
    if kind == "fall":
        s = placement_of(N, st)
        kw = dict(Q=len(st), tenure=3)
    else:
        pair = [_cell(N, 0, 1, 3), _cell(N, 0, 1, 5)]
        assert not set(pair) & set(st)
        s = placement_of(N, st[1:] + pair)
        tin = np.full((1, N ** 3), 50, dtype=np.uint16)
        tin[0, st[0]] = 0
        kw = dict(Q=len(st) + 1, tenure=3, tabu_in=tin, best_floor=np.zeros(1, dtype=np.int32))
    return s, ONE_SEED, 2, kw, tabu_many(N, s, ONE_SEED, 2, **kw)


@functools.lru_cache(maxsize=None)
def rho_case(N):
    """(placement, seeds, keywords, the restatement's result, (rho_q, rho_t)) of a move with the largest rho_q and rho_t of its shape:
    three queens in an L, so that the one at the corner is attacked twice and wins alone, as queen (o_q - 1) mod 3; the one cell that
    is not tabu is cell (o_t - 1) mod N^3, which none of the three attacks.  rho_t = N^3 - 1 takes all 15 bits at N = 32."""
    C = N ** 3
    oq, _, ot = draw(ONE_SEED[0], 0, N, 3, 0)
    q, t = (oq - 1) % 3, (ot - 1) % C
    for corner in range(C):
        i, j, k = corner // (N * N), (corner // N) % N, corner % N
        if k + 1 >= N or j + 2 >= N:
            continue
        trio = np.array([[i, j, k], [i, j, k + 1], [i, j + 2, k]], dtype=np.int64)
        if not attack_matrix(N, trio)[t].any():
            break
    order = [1, 2]
    order.insert(q, 0)  # the corner queen at index q
    s = trio[order].astype(np.uint8).reshape(1, -1)
    tin = np.full((1, C), 50, dtype=np.uint16)
    tin[0, t] = 0
    kw = dict(Q=3, tenure=3, tabu_in=tin, best_floor=np.zeros(1, dtype=np.int32))
    return s, ONE_SEED, kw, tabu_many(N, s, ONE_SEED, 2, **kw), (2, C - 1)


@functools.lru_cache(maxsize=None)
def full_cube_case(N=27):
    """(placement, seeds, Q, (queen, cell, delta, rho_q)) of the first move in a cube with ONE free cell t = (0, 1, 3), the queens in
    row-major order.  Queen q conflicts with every cell of its lines but t, so delta(q, t) = lines(t) - lines(q), the two corrections
    for t on q's lines cancelling; at odd N the centre alone has the most lines, 13 (N - 1), and wins alone.  Its index is large and the
    seed is the first whose o_q lies shortly behind it: rho_q >= 2^14 needs Q > 2^14, which fits the LDS from N = 26 on."""
    C = N ** 3
    t, centre = _cell(N, 0, 1, 3), _cell(N, N // 2, N // 2, N // 2)
    cells = [c for c in range(C) if c != t]
    q = cells.index(centre)
    lines_t = len(star(N, (0, 1, 3))) - 1
    seed = next(sd for sd in range(1, 1000) if (q - draw(sd, 0, N, C - 1, 0)[0]) % (C - 1) >= 1 << 14)
    return placement_of(N, cells), np.array([seed], dtype=np.uint32), C - 1, (q, t, lines_t - 13 * (N - 1), (q - draw(seed, 0, N, C - 1, 0)[0]) % (C - 1))
