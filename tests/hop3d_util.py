"""The basin-hopping rule of full_3d placements of include/mcq.h (mcq_hop3d) restated in NumPy and Python integers from the text of the
rule, on top of tests/quench3d_util.py and the Philox of tests/heatbath_util.py: what mcq_hop3d_host and the kernel are compared with.
A placement is a list of triples, a draw looks its cell up among them, E is never tracked but taken from L, and a rejected hop is
restored from a copy of the placement.

The local search is a parameter: "numpy" (the default) is quench3d_util.quench, which is slow beyond N = 4; "host" takes the library's
quench_queens_host with max_passes = 0, which rule item 2 says L is, so that the loop around L -- kick, accept, restore, best values,
counters -- can be restated at every N.  Either way the result carries `trace`, one entry per hop: "rejected", "same" (accepted on the
placement it left), "changed" or "improved" (changed, and below every energy before it), and the counts `occupied` (draws onto a cell
that holds a queen) and `drawn_twice` (hops whose kick drew some queen more than once)."""
import numpy as np

from tests import heatbath_util as hb
from tests import quench3d_util as q3

FIELDS = ("state", "energy_in", "energy_start", "energy_out", "best_energy", "best_hop", "best_state", "n_accepted", "n_improved", "n_moves",
          "n_passes", "n_kicked", "flags")
KEY_WORD = 6


def word(seed, w):
    """Word w (a Python integer below 2^63) of the hop stream of a chain seeded `seed`: rule item 4."""
    b = w >> 2
    return hb.philox((b & hb.MASK, b >> 32, 0, 0), (int(seed), KEY_WORD))[w & 3]


def kick_draws(N, Q, seed, g, m):
    """The (n, t) of the m draws of hop g, in order: a queen and a cell index."""
    out = []
    for d in range(m):
        x1, x2 = word(seed, 2 * (g * m + d)), word(seed, 2 * (g * m + d) + 1)
        out.append(((x1 * Q) >> 32, (x2 * N ** 3) >> 32))
    return out


def _search_numpy(N, z):
    """L on the clamped placement z (int64[Q][3]): (placement, E behind it, moves, passes)."""
    r = q3.quench(N, z, 0)
    return r["state"].astype(np.int64).reshape(-1, 3), int(r["energy_out"]), int(r["n_moves"]), int(r["n_passes"])


def _search_host(N, z):
    import mcq_amd

    r = mcq_amd.quench.quench_queens_host(N, z.astype(np.uint8).reshape(1, -1), Q=len(z), conflicts=False)
    return r["state"][0].astype(np.int64).reshape(-1, 3), int(r["energy_out"][0]), int(r["n_moves"][0]), int(r["n_passes"][0])


def hop(N, placement, seed, n_hops, kick=2, slack=0, first_hop=0, search="numpy"):
    """One placement through the rule; returns a dict with the fields of mcq_hop3d plus `energy_hist`, `trace`, `occupied`,
    `drawn_twice` and `kick`."""
    L = {"numpy": _search_numpy, "host": _search_host}[search]
    z = q3.clamp(N, placement).copy()
    Q = len(z)
    e_in = q3.energy(N, z)
    if q3.is_repeated(N, z):  # rule item 7
        st = z.astype(np.uint8).reshape(-1)
        return {"state": st, "best_state": st, "energy_in": e_in, "energy_start": e_in, "energy_out": e_in, "best_energy": e_in, "best_hop": 0,
                "n_accepted": 0, "n_improved": 0, "n_moves": 0, "n_passes": 0, "n_kicked": 0, "flags": 1,
                "energy_hist": np.full(n_hops + 1, e_in, dtype=np.int64), "trace": [], "occupied": 0, "drawn_twice": 0, "kick": kick}
    z, E, moves, passes = L(N, z)
    e_start = best = E
    best_hop, best_state = 0, z.copy()
    accepted = improved = kicked = occupied = twice = 0
    hist, trace = [E], []
    for t in range(n_hops):
        before = z.copy()  # the copy a rejected hop is restored from
        draws = kick_draws(N, Q, seed, first_hop + t, kick)
        twice += len({n for n, _ in draws}) < len(draws)
        for n, c in draws:
            cell = np.array([c // (N * N), (c // N) % N, c % N], dtype=np.int64)
            if (z == cell).all(axis=1).any():  # the cell holds a queen at this moment: nothing moves
                occupied += 1
                continue
            z[n] = cell
            kicked += 1
        z, e_new, m, p = L(N, z)
        moves, passes = moves + m, passes + p
        if e_new <= E + slack:
            accepted += 1
            E = e_new
            what = "same" if (z == before).all() else "changed"
            if E < best:
                best, best_hop, best_state = E, t + 1, z.copy()
                improved += 1
                what = "improved"
            trace.append(what)
        else:
            z = before
            trace.append("rejected")
        hist.append(E)
    return {"state": z.astype(np.uint8).reshape(-1), "energy_in": e_in, "energy_start": e_start, "energy_out": E, "best_energy": best,
            "best_hop": best_hop, "best_state": best_state.astype(np.uint8).reshape(-1), "n_accepted": accepted, "n_improved": improved,
            "n_moves": moves, "n_passes": passes, "n_kicked": kicked, "flags": 0, "energy_hist": np.array(hist, dtype=np.int64), "trace": trace,
            "occupied": occupied, "drawn_twice": twice, "kick": kick}


def hop_many(N, states, seeds, n_hops, Q=None, **kw):
    Q = N * N if Q is None else Q
    rows = [hop(N, s, int(sd), n_hops, **kw) for s, sd in zip(np.asarray(states).reshape(-1, 3 * Q), np.asarray(seeds).reshape(-1))]
    out = {k: np.stack([np.asarray(r[k]) for r in rows]) for k in FIELDS + ("energy_hist",)}
    out["trace"] = [r["trace"] for r in rows]
    out["occupied"] = sum(r["occupied"] for r in rows)
    out["drawn_twice"] = sum(r["drawn_twice"] for r in rows)
    out["kick"] = kw.get("kick", 2)
    return out


def assert_equal(got, want, what, hist=True):
    for k in FIELDS + (("energy_hist",) if hist else ()):
        g, w = np.asarray(got[k]).astype(np.int64), np.asarray(want[k]).astype(np.int64)
        np.testing.assert_array_equal(g.reshape(w.shape), w, err_msg=f"{what}: {k}")


class Coverage:
    """The condition on the inputs: what the restatement's traces of a group of comparisons contain.  A group without rejected hops
    never ran the restore path, one without accepted hops on a changed placement never ran the commit path, one without a draw onto an
    occupied cell never refused a draw, and one without a queen drawn twice never moved a queen the kick had moved already."""

    def __init__(self):
        self.count = {}

    def add(self, group, want):
        c = self.count.setdefault(group, {"rejected": 0, "changed": 0, "improved": 0, "hops": 0, "occupied": 0, "drawn_twice": 0})
        c["occupied"] += want["occupied"]
        c["drawn_twice"] += want["drawn_twice"]
        for tr in want["trace"]:
            c["hops"] += len(tr)
            c["rejected"] += tr.count("rejected")
            c["changed"] += tr.count("changed") + tr.count("improved")
            c["improved"] += tr.count("improved")

    def check(self, group):
        c = self.count[group]
        assert c["rejected"] >= 3 and c["changed"] >= 3 and c["improved"] >= 1 and c["occupied"] >= 1 and c["drawn_twice"] >= 1, (group, c)
        return c


def is_local_minimum(N, placement):
    """quench3d_util.is_local_minimum's property -- no queen has a free cell with a lower count than the one it holds -- from ONE attack
    matrix of cells x queens: a(q, t) is its row sum less queen q's own entry.  quench3d_util's function rebuilds the matrix per queen,
    which takes seconds at N = 13 and minutes at N = 20; tests/test_hop3d_host.py holds the two against each other on minima and on
    placements that are none."""
    z = q3.clamp(N, placement)
    att = q3.attack_matrix(q3._cells(N), z)
    total = att.sum(axis=1, dtype=np.int64)
    idx = (z[:, 0] * N + z[:, 1]) * N + z[:, 2]
    taken = np.zeros(N ** 3, dtype=bool)
    taken[idx] = True
    for q in range(len(z)):
        a = total - att[:, q]
        free = ~taken
        free[idx[q]] = True  # its own cell is a candidate
        if a[free].min() < a[idx[q]]:
            return False
    return True


def mark_first_hop(kick, before=2):
    """A first_hop `before` hops short of the hop whose kick holds word 2^35 of the stream: there w >> 34, the second counter word of the
    block of word w, goes from 1 to 2 (rule item 4: the high bits of w / 4)."""
    return (1 << 35) // (2 * kick) - before


def crosses_the_mark(kick, first_hop, n_hops):
    return (2 * kick * first_hop) >> 34 == 1 and (2 * kick * (first_hop + n_hops) - 1) >> 34 == 2


def merge(parts):
    """The figures of a run cut into the calls `parts` (in order, each fed the `state` of the one before and first_hop carried over):
    n_accepted, n_moves and n_kicked add up, and so does n_passes less the one moveless pass with which every later call finds its input
    to be a minimum; energy_in / energy_start are the first call's, state / energy_out the last call's, best_* those of the FIRST call
    with the smallest best_energy, its best_hop moved by the hops before that call; the histories are joined without the repeated first
    entry, and n_improved counts the new lows of the joined history."""
    out = {"state": parts[-1]["state"], "energy_out": parts[-1]["energy_out"], "energy_in": parts[0]["energy_in"], "energy_start": parts[0]["energy_start"],
           "flags": parts[0]["flags"]}
    for k in ("n_accepted", "n_moves", "n_kicked", "n_passes"):
        out[k] = sum(np.asarray(p[k]).astype(np.int64) for p in parts)
    out["n_passes"] = out["n_passes"] - (len(parts) - 1)
    be = np.stack([np.asarray(p["best_energy"]).astype(np.int64) for p in parts])
    first = be.argmin(axis=0)  # the first of the smallest
    n_hops = [p["energy_hist"].shape[1] - 1 for p in parts]
    before = np.concatenate([[0], np.cumsum(n_hops)[:-1]])
    rows = np.arange(be.shape[1])
    out["best_energy"] = be[first, rows]
    out["best_hop"] = np.stack([np.asarray(p["best_hop"]).astype(np.int64) for p in parts])[first, rows] + before[first]
    out["best_state"] = np.stack([p["best_state"] for p in parts])[first, rows]
    out["energy_hist"] = np.concatenate([parts[0]["energy_hist"]] + [p["energy_hist"][:, 1:] for p in parts[1:]], axis=1)
    low = np.minimum.accumulate(out["energy_hist"].astype(np.int64), axis=1)
    out["n_improved"] = (low[:, 1:] < low[:, :-1]).sum(axis=1)
    return out
