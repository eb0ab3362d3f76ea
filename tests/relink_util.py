"""The path-relinking rule of include/mcq.h (mcq_relink) restated in NumPy and Python integers from the text of the rule and nothing else,
on top of the table of tests/tabu_util.py, the Philox of tests/heatbath_util.py and the local searches of tests/quench_util.py and
tests/quench_pairs_util.py: what mcq_relink_host and the kernel are compared with.  a(c, k) is recounted before every step, and every
placement of the walk is kept, so that P* is picked from the list behind the walk and not along it.

The local search is the restatement's own up to N = 8 and the library's quench host calls beyond (search="host"), as in
tests/hop_util.py.  Every step leaves a trace: delta, the number of ties, whether the column taken was not the smallest tied one, whether
rho wrapped (the column taken lies below the offset o), whether the placement behind the step was a candidate and whether it was a new
P*."""
import functools

import numpy as np

from tests import heatbath_util as hb
from tests import hop_util as hu
from tests import quench_util as qu
from tests import tabu_util as tu

FIELDS = ("state", "path_best_state", "distance_in", "n_steps", "path_best_step", "energy_in", "path_best_energy", "path_max_energy",
          "energy_out", "n_moves", "n_pair_moves")
KEY_WORD = 9
NUMPY_MAX_N = 8  # the restatement's own local search up to here


def offset(seed, t, walk, N):
    """o of step t of walk `walk`: rule item 2."""
    x = hb.philox((t, walk & hb.MASK, walk >> 32, 0), (int(seed), KEY_WORD))
    return (x[0] * N * N) >> 32


def energy(N, h):
    return int(tu.table(N, h)[np.arange(N * N), h].sum()) // 2


@functools.lru_cache(maxsize=None)
def _walk(N, hb_, gb_, seed, max_steps, walk):
    """The walk of rule item 2 between two clamped placements (as bytes): (every placement of the path, their energies, the steps' traces).
    Computed once per pair and shared between the calls that differ in min_dist or in the local search alone."""
    Q = N * N
    h, g = np.frombuffer(hb_, dtype=np.int64).copy(), np.frombuffer(gb_, dtype=np.int64)
    e_in = energy(N, h)
    d0 = int((h != g).sum())
    n_steps = d0 if max_steps == 0 else min(d0, max_steps)
    path, energies, trace = [h.copy()], [e_in], []
    E = e_in
    for t in range(n_steps):
        o = offset(seed, t, walk, N)
        a = tu.table(N, h)
        F = np.nonzero(h != g)[0]
        delta = a[F, g[F]] - a[F, h[F]]
        rho = (F - o) % Q
        dmin = int(delta.min())
        ties = F[delta == dmin]
        c = int(ties[np.argmin(rho[delta == dmin])])
        h[c] = g[c]
        E += dmin
        path.append(h.copy())
        energies.append(E)
        trace.append({"delta": dmin, "ties": len(ties), "not_first": c != int(ties.min()), "wrapped": c < o, "o": o, "c": c})
    assert E == energy(N, h)  # the sum of the deltas is the recount's difference
    return path, energies, trace


def relink(N, board, guide, seed, max_steps=0, min_dist=1, local_search="pairs", walk=0, search=None):
    """One chain through the rule; returns a dict with the fields of mcq_relink plus `energy_hist` (W + 1 entries) and `trace`."""
    Q = N * N
    search = search or ("numpy" if N <= NUMPY_MAX_N else "host")
    L = {"numpy": hu._search_numpy, "host": hu._search_host}[search]
    h, g = qu.clamp(N, board).copy(), qu.clamp(N, guide)
    d0 = int((h != g).sum())
    n_steps = d0 if max_steps == 0 else min(d0, max_steps)
    W = max_steps if max_steps else Q
    path, energies, trace = _walk(N, h.astype(np.int64).tobytes(), g.astype(np.int64).tobytes(), int(seed), max_steps, walk)
    trace = [dict(s) for s in trace]
    e_in = energies[0]
    # the candidates, from the list: t counted from 1
    cands = [t for t in range(1, n_steps + 1) if t >= max(1, min_dist) and d0 - t >= min_dist]
    low = None
    for t in cands:
        trace[t - 1]["candidate"] = True
        if low is None or energies[t] < energies[low]:
            low = t
            trace[t - 1]["new_low"] = True
    best_step = low or 0
    pstar = path[best_step]
    hs, e_out, moves, pair_moves = L(N, pstar.copy(), local_search == "pairs")
    hist = energies + [energies[-1]] * (W - n_steps)
    return {"state": hs.astype(np.uint8), "path_best_state": pstar.astype(np.uint8), "distance_in": d0, "n_steps": n_steps, "path_best_step": best_step,
            "energy_in": e_in, "path_best_energy": energies[best_step], "path_max_energy": max(energies), "energy_out": e_out, "n_moves": moves,
            "n_pair_moves": pair_moves, "energy_hist": np.array(hist, dtype=np.int64), "trace": trace, "n_candidates": len(cands),
            "energy_guide": energy(N, g)}


def relink_many(N, states, guides, seeds, **kw):
    states, guides = np.asarray(states).reshape(-1, N * N), np.asarray(guides).reshape(-1, N * N)
    rows = [relink(N, s, g, int(sd), **kw) for s, g, sd in zip(states, guides, np.asarray(seeds).reshape(-1))]
    out = {k: np.stack([np.asarray(r[k]) for r in rows]) for k in FIELDS + ("energy_hist", "n_candidates", "energy_guide")}
    out["trace"] = [r["trace"] for r in rows]
    out["min_dist"] = kw.get("min_dist", 1)
    return out


def host_cover(N, got, guides, min_dist):
    """The host code's outputs with what Coverage.add needs beside them: the number of candidates from rule item 3 and the guides'
    energies from the host quench's recount."""
    import mcq_amd

    out = dict(got)
    first, last = max(1, min_dist), np.minimum(got["n_steps"].astype(np.int64), got["distance_in"].astype(np.int64) - min_dist)
    out["n_candidates"] = np.maximum(0, last - first + 1)
    out["energy_guide"] = mcq_amd.quench.quench_states_host(N, guides, max_passes=1, conflicts=False)["energy_in"]
    out["min_dist"] = min_dist
    return out


def assert_equal(got, want, what, fields=FIELDS + ("energy_hist",), rows=None):
    for k in fields:
        a, b = np.asarray(got[k]).astype(np.int64), np.asarray(want[k]).astype(np.int64)
        if rows is not None:
            a = a[rows]
        np.testing.assert_array_equal(a, b, err_msg=f"{what}: {k}")


def minima(N, n, seed):
    """n single-move minima of random boards, by the library's host quench.  Inputs only: whatever the host code returns, the host
    code, the kernel and the restatement must agree on what follows."""
    import mcq_amd

    return mcq_amd.quench.quench_states_host(N, qu.random_boards(N, n, seed), conflicts=False)["state"]


def neighbours(states):
    """Each placement's guide: the next one in the list."""
    return np.roll(np.asarray(states), -1, axis=0)


class Coverage:
    """What a group of compared calls (one instantiation of the kernel) must contain before a comparison counts: from the restatement's
    traces and outputs, or from the host code's outputs where the restatement is too slow, never from the kernel's."""

    NEED = {"not_first": 5, "wrapped": 10, "rise": 10, "fall": 5, "inside": 1, "at_last_candidate": 2, "no_candidate": 4, "search_moved": 10,
            "search_still": 4, "pair_move": 10, "below_both": 10}

    def __init__(self):
        self.count = {}

    def add_traces(self, group, traces):
        """The steps' traces of relink_many's result."""
        c = self.count.setdefault(group, dict.fromkeys(self.NEED, 0))
        for tr in traces:
            for s in tr:
                c["not_first"] += s["ties"] >= 2 and s["not_first"]
                c["wrapped"] += s["wrapped"]
                c["rise"] += s["delta"] > 0
                c["fall"] += s["delta"] < 0

    def add_outputs(self, group, want):
        """`want`: relink_many's result, or the host code's outputs through host_cover."""
        c = self.count.setdefault(group, dict.fromkeys(self.NEED, 0))
        d0, step, n_steps = (np.asarray(want[k]).astype(np.int64) for k in ("distance_in", "path_best_step", "n_steps"))
        ncand = np.asarray(want["n_candidates"]).astype(np.int64)
        last = np.minimum(n_steps, d0 - want["min_dist"])  # the t of the last candidate
        c["inside"] += int(((step > max(1, want["min_dist"])) & (step < last)).sum())
        c["at_last_candidate"] += int(((step > 0) & (step == last) & (ncand >= 2)).sum())
        c["no_candidate"] += int(((ncand == 0) & (n_steps > 0)).sum())
        moved = np.asarray(want["n_moves"]).astype(np.int64) + np.asarray(want["n_pair_moves"]).astype(np.int64)
        c["search_moved"] += int((moved > 0).sum())
        c["search_still"] += int((moved == 0).sum())
        c["pair_move"] += int((np.asarray(want["n_pair_moves"]) > 0).sum())
        e_out = np.asarray(want["energy_out"]).astype(np.int64)
        c["below_both"] += int(((e_out < np.asarray(want["energy_in"])) & (e_out < np.asarray(want["energy_guide"])) & (d0 > 0)).sum())

    def check(self, group, pairs=True):
        c = self.count[group]
        for k, need in self.NEED.items():
            if k == "pair_move" and not pairs:
                continue
            assert c[k] >= need, (group, k, c)
        return c
