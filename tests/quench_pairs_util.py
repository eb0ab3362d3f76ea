"""The pair-move quench rule of include/mcq.h (mcq_quench_pairs) restated in NumPy from the text of the rule, on top of
tests/quench_util.py: what mcq_quench_pairs_host and the kernel are compared with.  The scan here goes over ALL pairs of columns,
aligned or not, and skips no candidate; for N <= 4 it takes D from a full recount of the energy instead of the formula.  It is
therefore independent of both shortcuts the library may take.

fast_scan is the same rule item 3 vectorised per first column: every aligned pair, every (k1, k2), nothing pruned by difference.  It is
what makes the restatement reach N = 32; it leaves the non-aligned pairs out, which is sound only on a single-move minimum (their D is a
sum of two differences >= 0), so whoever takes it as a certificate asserts qu.is_local_minimum next to it.  tests/test_quench_pairs_host.py
pins it to the slow scans.  quench_pairs records a `trace` of its pair moves, and Coverage states what a set of inputs must contain."""
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


@functools.lru_cache(maxsize=None)
def _partners(N):
    """Per column c1: (the aligned columns c2 > c1 in ascending order, their d), from geometry."""
    aligned, d = geometry(N)
    out = []
    for c1 in range(N * N):
        c2 = np.flatnonzero(aligned[c1, c1 + 1:]) + c1 + 1
        out.append((c2, d[c1, c2]))
    return out


def fast_scan(N, h, t=None):
    """The lexicographically smallest (D, c1, c2, k1, k2) over ALL candidates of rule item 3 -- every aligned pair c1 < c2, every k1 != h(c1)
    and k2 != h(c2) --, from the formula of the rule on the table a(c, k) of tests/quench_util.py: one array [c2][k1][k2] per c1."""
    h = np.asarray(h, dtype=np.int64)
    t = qu.table(N, h) if t is None else t
    delta = (t - t[np.arange(N * N), h][:, None]).astype(np.int16)  # the single-move differences: |delta| <= 4 (N - 1)
    k = np.arange(N, dtype=np.int16)
    z = np.abs(k[:, None] - k[None, :])
    both = np.stack([(z == 0) | (z == d) for d in range(N)]).astype(np.int16)  # att((., k1), (., k2)) by distance
    none = 10000  # what stands for "no candidate": above every D, and two of them still fit int16
    best = None
    for c1 in range(N * N - 1):
        c2, d = _partners(N)[c1]
        if c2.size == 0:
            continue
        h1, h2 = int(h[c1]), h[c2]
        first = delta[c1][None, :] - both[d, :, h2] + both[d, h1, h2][:, None]  # [c2][k1]: a(c1, k1) - a(c1, h1) - att(k1, h2) + att(h1, h2)
        second = delta[c2] - both[d, h1, :]                                     # [c2][k2]: a(c2, k2) - a(c2, h2) - att(h1, k2)
        first[:, h1] = none
        second[np.arange(c2.size), h2] = none
        D = both[d]  # [c2][k1][k2]: att(k1, k2), a copy
        D += first[:, :, None]
        D += second[:, None, :]
        m = int(D.min())
        if m >= none or (best is not None and m >= best[0]):
            continue  # c1 ascends: a tie with an earlier column loses
        w, k1, k2 = np.argwhere(D == m)[0]  # row-major: the smallest (c2, k1, k2)
        best = (m, c1, int(c2[w]), int(k1), int(k2))
    return best


FAMILIES = ("row", "column", "diagonal", "antidiagonal")


def family(N, c1, c2):
    """Which line of the board the aligned columns c1, c2 share."""
    (i1, j1), (i2, j2) = divmod(c1, N), divmod(c2, N)
    return "row" if i1 == i2 else "column" if j1 == j2 else "diagonal" if i2 - i1 == j2 - j1 else "antidiagonal"


def lane_slot(N, c1, c2):
    """The index 0 .. 4 N - 1 under which a lane loop over (row, board column, diagonal, antidiagonal) x position meets c2 from c1: the
    position is the row index along the board column and the column index along the three others.  From 64 on it is a wavefront's
    second trip."""
    f = FAMILIES.index(family(N, c1, c2))
    return f * N + (c2 // N if f == 1 else c2 % N)


def descend(N, h):
    """Passes of the single-move rule until one moves nothing; returns (heights, energy drop, moves)."""
    r = qu.quench(N, h)
    return r["state"].astype(np.int64), r["energy_in"] - r["energy_out"], r["n_moves"]


def quench_pairs(N, board, max_rounds=0, pairs="all", delta=None):
    """One board through the rule; returns a dict with the fields of mcq_quench_pairs plus `deltas`, the D of the pair moves, and `trace`,
    one dict per pair move: D, d1, d2 (the single-move differences of k1 and k2), family, slot, c1, c2, k1, k2.  pairs="fast" takes
    fast_scan (every scan of a run sits behind a descent, so leaving the non-aligned pairs out changes nothing)."""
    h = qu.clamp(N, board).copy()
    e_in = qu.energy(N, h)
    h, drop, moves = descend(N, h)
    E = e_single = e_in - drop
    rounds = pair_moves = certified = 0
    deltas, trace = [], []
    while True:
        rounds += 1
        t = qu.table(N, h)
        D, c1, c2, k1, k2 = fast_scan(N, h, t) if pairs == "fast" else scan(N, h, pairs, delta)
        if D >= 0:
            certified = 1
            break
        trace.append({"D": D, "d1": int(t[c1][k1] - t[c1][h[c1]]), "d2": int(t[c2][k2] - t[c2][h[c2]]), "family": family(N, c1, c2),
                      "slot": lane_slot(N, c1, c2), "c1": c1, "c2": c2, "k1": k1, "k2": k2})
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
            "conflicts": t[np.arange(N * N), h].astype(np.uint16), "deltas": deltas, "trace": trace}


def quench_pairs_many(N, states, max_rounds=0, **kw):
    rows = [quench_pairs(N, s, max_rounds, **kw) for s in np.asarray(states).reshape(-1, N * N)]
    out = {k: np.stack([np.asarray(r[k]) for r in rows]) for k in FIELDS}
    out["deltas"] = [r["deltas"] for r in rows]
    out["trace"] = [r["trace"] for r in rows]
    return out


def assert_equal(got, want, what):
    for k in FIELDS:
        np.testing.assert_array_equal(np.asarray(got[k]).astype(np.int64), np.asarray(want[k]).astype(np.int64), err_msg=f"{what}: {k}")


CLASSES = ((-2, 0, 0), (-1, 0, 0), (-1, 1, 0), (-1, 0, 1))  # (D, d1, d2); D < 0 with d1, d2 >= 0 and the att terms >= -2 admits no other


def padded(N):
    """The edge the kernels pad N to: their instantiations."""
    return next(p for p in (4, 8, 12, 16, 24, 32) if N <= p)


def kicked_minima(N, n, seed, kick):
    """n boards a few pair moves away from a minimum: random boards converged once by the library's host code, then `kick` columns of
    each redrawn.  Inputs only -- whatever the host code returns, host code, kernel and restatement must agree on what follows.  Heights
    N - 1 come as 255."""
    import mcq_amd

    s = mcq_amd.quench.quench_pairs_host(N, qu.random_boards(N, n, seed), conflicts=False)["state"].copy()
    rs = np.random.RandomState(seed + 1)
    for r in range(n):
        s[r, rs.choice(N * N, size=kick, replace=False)] = rs.randint(0, N, size=kick)
    s[s == N - 1] = 255
    return s


# The inputs on which host code, kernel and restatement are compared at both ends of every instantiation.  Seeds, counts and kicks were
# chosen on the CPU so that the restatement's traces alone meet Coverage.check; nothing the library computes entered the choice.
GROUPS = {4: (2, 4), 8: (5, 8), 12: (9, 12), 16: (13, 16), 24: (17, 24), 32: (25, 32)}
RANDOM_CASES = {2: (6, 302), 4: (12, 324), 5: (6, 305), 8: (5, 308), 9: (3, 309), 12: (4, 312), 13: (3, 323), 16: (3, 326)}  # N: (boards, seed)
KICKED_CASES = {17: (3, 1, 12), 24: (3, 1, 24), 25: (3, 0, 12), 32: (3, 4, 12)}  # N: (boards, seed, columns redrawn)


def random_case_boards(N):
    n, seed = RANDOM_CASES[N]
    s = qu.random_boards(N, n, seed, over=True)  # bytes >= N among them
    s[0] = seed % N  # all heights equal
    s[1] = 255       # every byte clamped
    return s


@functools.lru_cache(maxsize=None)
def restated_case(N):
    """(boards, the restatement's run to convergence with fast_scan) of the comparison at N: random boards up to N = 16, kicked minima
    beyond, where a run from a random board takes the restatement a minute.  Computed once per session, shared and left unchanged."""
    s = random_case_boards(N) if N in RANDOM_CASES else kicked_minima(N, *KICKED_CASES[N])
    s.setflags(write=False)
    return s, quench_pairs_many(N, s, pairs="fast")


def certify(N, board, what=""):
    """The certificate of a 2-move minimum that owes nothing to the library: no single move lowers E (so no pair of columns that are not
    aligned does), and no candidate of rule item 3 has D < 0."""
    h = qu.clamp(N, board)
    assert qu.is_local_minimum(N, h), f"{what}: a single move lowers E"
    best = fast_scan(N, h)
    assert best[0] >= 0, f"{what}: the pair move (D, c1, c2, k1, k2) = {best} lowers E"


class Coverage:
    """The condition on the inputs of a group of comparisons (one instantiation), from the restatement's traces: a comparison whose runs
    never take a pair move of some class, along some line, at the last heights of a table row or on the second trip of a lane loop says
    nothing about the code that handles it."""

    def __init__(self):
        self.seen = {}

    def add(self, N, want):
        c = self.seen.setdefault(padded(N), {"classes": set(), "families": set(), "N": 0, "moves": 0, "most_rounds": 0})
        if N > c["N"]:
            c.update(N=N, last_dword=0, uphill_last_dword=0, top_height=0)
        for tr in want["trace"]:
            c["moves"] += len(tr)
            c["most_rounds"] = max(c["most_rounds"], len(tr) + 1)
            for m in tr:
                c["classes"].add((m["D"], m["d1"], m["d2"]))
                c["families"].add(m["family"])
                c["second_trip"] = c.get("second_trip", 0) + (m["slot"] >= 64)
                c["neighbours"] = c.get("neighbours", 0) + (m["c2"] == m["c1"] + 1)
                if N == c["N"]:  # the group's largest N so far
                    last = padded(N) - 4
                    c["last_dword"] += m["k1"] >= last or m["k2"] >= last
                    c["uphill_last_dword"] += (m["d1"] == 1 and m["k1"] >= last) or (m["d2"] == 1 and m["k2"] >= last)
                    c["top_height"] += N - 1 in (m["k1"], m["k2"])

    def check(self, NP, N, classes=CLASSES):
        """The group NP must have been fed its largest N = `N`; `classes` are those it must hold (a test that excepts one names it)."""
        c = self.seen[NP]
        assert c["N"] == N and set(c["classes"]) <= set(CLASSES), (NP, c)
        assert set(classes) <= c["classes"], (NP, "classes missing", set(classes) - c["classes"], c)
        assert c["families"] == set(FAMILIES), (NP, c)
        assert c["last_dword"] >= 1 and c["top_height"] >= 1 and c["neighbours"] >= 1 and c["most_rounds"] >= 3, (NP, c)
        if set(classes) & {(-1, 1, 0), (-1, 0, 1)}:
            assert c["uphill_last_dword"] >= 1, (NP, c)  # the height that costs 1 sits in the last dword of its row's mask
        if N > 16:
            assert c["second_trip"] >= 1, (NP, c)
        return c


def has_improving_pair_by_recount(N, board):
    h = qu.clamp(N, board)
    return scan(N, h, "all", "recount")[0] < 0
