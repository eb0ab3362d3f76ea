"""The inputs that tests/test_relink3d_host.py and tests/test_relink3d.py share: per shape (N, Q) a list of named cases -- minima relinked
with their neighbour, random placements with bytes >= N, a guide that is the placement with its queens permuted, disjoint placements,
windows of one candidate and of none, a guide that is a candidate itself, a walk cut below min_dist and a cut walk --, the host code's
result and the restatement's, each computed once, shared and left unchanged; the tally that a group of compared calls has to hold
before its comparisons count; and the placements at the ends of the kernel's packed key."""
import functools

import numpy as np

import mcq_amd
from tests import quench3d_util as q3
from tests import relink3d_util as ru
from tests import tabu3d_util as t3

abi = mcq_amd.abi
quench = mcq_amd.quench


def queens_of(N, Q):
    return N * N if Q is None else Q


def room(N, Q):
    """The largest d0 of a shape: the queens, or the free cells when those are fewer."""
    Q = queens_of(N, Q)
    return min(Q, N ** 3 - Q)


def minima(N, n, seed, Q=None):
    return quench.quench_queens_host(N, q3.random_placements(N, n, seed, Q=Q), Q=Q, conflicts=False)["state"]


def toward(N, s, d, seed, Q=None):
    """Guides at set distance d from the placements s (clamped): d queens of each replaced by cells that hold none."""
    Q = queens_of(N, Q)
    rs = np.random.RandomState(seed)
    z = np.minimum(s.reshape(len(s), Q, 3), N - 1).astype(np.int64)
    g = z.copy()
    for r in range(len(s)):
        idx = (z[r, :, 0] * N + z[r, :, 1]) * N + z[r, :, 2]
        free = np.setdiff1d(np.arange(N ** 3), idx)
        cells = rs.choice(free, size=d, replace=False)
        g[r, rs.choice(Q, size=d, replace=False)] = np.stack([cells // (N * N), (cells // N) % N, cells % N], axis=1)
    return g.astype(np.uint8).reshape(len(s), -1)


def permuted(s, seed, Q):
    rs = np.random.RandomState(seed)
    return np.stack([row.reshape(Q, 3)[rs.permutation(Q)].reshape(-1) for row in s])


@functools.lru_cache(maxsize=None)
def cases(N, Q=None, n=4, few=False):
    """((name, placements, guides, seeds, keywords), ..) of a shape.  few=True is for the shapes where a step of the restatement is a
    matrix of millions: the two whole walks between minima and between disjoint placements stay, the walk between random placements
    goes, and the windows and cuts are set on guides a few moves away."""
    Qn, D = queens_of(N, Q), room(N, Q)
    seeds = abi.seeds_for(1000 * N + Qn, n)
    m = minima(N, n + 1, 7 * N + Qn, Q=Q)
    rnd, rnd2 = q3.random_placements(N, n, 11 * N + Qn, Q=Q, over=True), q3.random_placements(N, n, 13 * N + Qn, Q=Q, over=True)
    md = max(1, Qn // 8)
    out = [("minima", m[:n], m[1:], seeds, dict(min_dist=min(md, Qn)))]
    if not few:
        out.append(("random, bytes >= N", rnd, rnd2, seeds, dict(min_dist=1)))
    if 2 * Qn <= N ** 3:
        far = q3.random_placements(N, n, 17 * N + Qn, Q=2 * Qn).reshape(n, 2, -1)  # 2 Q distinct cells: no cell shared
        out.append(("disjoint", far[:, 0].copy(), far[:, 1].copy(), seeds, dict(min_dist=min(md, Qn))))
    quarter = max(1, min(D // 4, 3) if few else D // 4)
    near = toward(N, rnd, min(D, 9), 29 * N + Qn, Q=Q) if few else rnd2
    out += [("the guide is the placement, permuted", rnd, permuted(rnd, N + Qn, Qn), seeds, dict(min_dist=1)),
            ("the guide a candidate", m[:n], toward(N, m[:n], min(D, 7), 31 * N + Qn, Q=Q) if few else m[1:], seeds, dict(min_dist=0)),
            ("one step, below min_dist", rnd, near, seeds, dict(max_steps=1, min_dist=min(2, Qn))),
            ("a cut walk", rnd, near, seeds, dict(max_steps=max(1, min(D, 9) // 3 if few else D // 3), min_dist=1)),
            ("no candidate", rnd, toward(N, rnd, max(1, 2 * quarter - 1), 19 * N + Qn, Q=Q), seeds, dict(min_dist=quarter))]
    if 2 * quarter <= D:
        out.append(("one candidate", rnd, toward(N, rnd, 2 * quarter, 23 * N + Qn, Q=Q), seeds, dict(min_dist=quarter)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def hosted(N, Q, n, few, i):
    name, s, g, seeds, kw = cases(N, Q, n, few)[i]
    return quench.relink_queens_host(N, s, g, seeds, Q=Q, hist=True, **kw)


@functools.lru_cache(maxsize=None)
def restated(N, Q, n, few, i, rows=None):
    """The restatement of case i: every chain (rows=None) or the first `rows`."""
    name, s, g, seeds, kw = cases(N, Q, n, few)[i]
    return ru.relink_many(N, s, g, seeds, Q=Q, rows=None if rows is None else slice(0, rows), **kw)


def with_last_candidate(host, kw):
    """The host outputs with the step of the last candidate of every chain (0: no candidate), for ru.tally."""
    md = kw.get("min_dist", 1)
    d0, steps = np.asarray(host["distance_in"]).astype(np.int64), np.asarray(host["n_steps"]).astype(np.int64)
    last = np.minimum(d0 - md, steps)
    return dict(host, last_candidate=np.where(last >= max(1, md), last, 0))


def tally(shapes, rows=None):
    """The sum of ru.tally over the cases of `shapes` ((N, Q, n, few), ..), from the restatement's traces and the host code's outputs."""
    total = {}
    for N, Q, n, few in shapes:
        for i, (name, s, g, seeds, kw) in enumerate(cases(N, Q, n, few)):
            want, host = restated(N, Q, n, few, i, rows), hosted(N, Q, n, few, i)
            k = len(want["trace"])
            part = ru.tally(want["trace"], {f: np.asarray(v)[:k] for f, v in with_last_candidate(host, kw).items()}, minima=name == "minima")
            for f, v in part.items():
                total[f] = total.get(f, 0) + int(v)
    return total


def check_tally(t, what):
    """The coverage that a group of compared calls holds, or an AssertionError naming what is missing."""
    need = ("ties", "wrapped_q", "wrapped_t", "rises", "falls", "on_line", "off_line", "pstar_inside", "pstar_last", "pstar_absent", "l_moves", "l_still",
            "below_both")
    missing = [k for k in need if t.get(k, 0) < 1]
    assert not missing, f"{what}: the compared calls hold no {missing}: {t}"
    return t


# ---- the ends of the packed key (delta + 403) << 30 | rho_q << 15 | rho_t ----
KEY_N = {19: 234, 32: 397}  # N -> the size of the largest fall and rise: the queens of the star that attack its centre
ONE_SEED = np.array([12345], dtype=np.uint32)


@functools.lru_cache(maxsize=None)
def key_case(N):
    """(A, G, Q, c): A is the star of the centre (tests/tabu3d_util.star) and two fillers, G is A with the centre queen on a cell c that no
    queen of A attacks.  d0 = 1: the one step moves the centre queen to c and delta = -(the star's other queens); with A and G
    exchanged the queen returns and delta is as large as a rise gets."""
    st = t3.star(N)
    z = t3.placement_of(N, st).reshape(-1, 3).astype(np.int64)
    seen = t3.attack_matrix(N, z).any(axis=1)
    c = int(np.flatnonzero(~seen)[0])
    cz = t3.placement_of(N, [c]).reshape(1, 3).astype(np.int64)
    quiet = ~t3.attack_matrix(N, cz)[:, 0]  # cells that do not attack c
    quiet[st] = False
    quiet[c] = False
    fillers = [int(x) for x in np.flatnonzero(quiet)[:2]]
    a = t3.placement_of(N, st + fillers)
    g = t3.placement_of(N, [c] + st[1:] + fillers)
    return a, g, len(st) + 2, c


@functools.lru_cache(maxsize=None)
def rho_case(N, Q=3):
    """(A, G, Q, (q, t)) of a walk of one step whose winner has rho_q = Q - 1 and rho_t = N^3 - 1, from the restatement's o_q and o_t:
    queen (o_q - 1) mod Q alone stands off the guide, and the guide's one open cell is (o_t - 1) mod N^3."""
    C = N ** 3
    oq, ot = ru.draw(ONE_SEED[0], 0, 0, N, Q)
    q, t = (oq - 1) % Q, (ot - 1) % C
    cells = [c for c in (5, 77, 1234 % C, 999 % C, 4321 % C) if c != t][:Q]
    a = t3.placement_of(N, cells)
    gc = list(cells)
    gc[q] = t
    return a, t3.placement_of(N, gc), Q, (q, t)


@functools.lru_cache(maxsize=None)
def full_cube_case(N=27):
    """(A, G, seeds, Q, (q, t, rho_q)): the cube with ONE free cell t, the queens in row-major order; the guide frees the cell of a queen
    q instead, so q alone moves, to t.  The seed is the first whose o_q puts rho_q at or above 2^14, which needs Q > 2^14."""
    C = N ** 3
    Q = C - 1
    t = (0 * N + 1) * N + 3
    cells = [c for c in range(C) if c != t]
    q = Q - 5
    seed = next(sd for sd in range(1, 1000) if (q - ru.draw(sd, 0, 0, N, Q)[0]) % Q >= 1 << 14)
    gc = [c for c in range(C) if c != cells[q]]
    return t3.placement_of(N, cells), t3.placement_of(N, gc), np.array([seed], dtype=np.uint32), Q, (q, t, (q - ru.draw(seed, 0, 0, N, Q)[0]) % Q)
