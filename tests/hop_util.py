"""The basin-hopping rule of include/mcq.h (mcq_hop) restated in NumPy and Python integers from the text of the rule, on top of
tests/quench_util.py, tests/quench_pairs_util.py and the Philox of tests/heatbath_util.py: what mcq_hop_host and the kernel are compared
with.  a(c, k) is recounted naively per use, the pair scan visits ALL pairs of columns and skips no candidate, and a rejected hop is
restored from a copy of the placement.

The local search is a parameter: "numpy" (the default) is the restatement's own, which is slow beyond N = 8; "host" takes the
library's quench host calls (mcq_quench_host with max_passes = 0, mcq_quench_pairs_host with max_rounds = 0), which rule item 8
says L is, so that the loop around L -- kick, accept, restore, best values, counters -- can be restated at every N.  Either way the
result carries `trace`, one entry per hop: "rejected", "same" (accepted on the placement it left), "changed" or "improved" (changed,
and below every energy before it)."""
import numpy as np

from tests import heatbath_util as hb
from tests import quench_pairs_util as qp
from tests import quench_util as qu

FIELDS = ("state", "energy_in", "energy_start", "energy_out", "best_energy", "best_hop", "best_state", "n_accepted", "n_improved", "n_moves",
          "n_pair_moves")
KEY_WORD = 5


def word(seed, w):
    """Word w (a Python integer below 2^63) of the hop stream of a chain seeded `seed`: rule item 4."""
    b = w >> 2
    return hb.philox((b & hb.MASK, b >> 32, 0, 0), (int(seed), KEY_WORD))[w & 3]


def kick_draws(N, seed, g, m):
    """The (c, k) of the m draws of hop g, in order."""
    out = []
    for q in range(m):
        x1, x2 = word(seed, 2 * (g * m + q)), word(seed, 2 * (g * m + q) + 1)
        out.append(((x1 * N * N) >> 32, (x2 * N) >> 32))
    return out


def _search_numpy(N, h, pairs):
    """L on the clamped heights h: (heights, E behind it, single moves, pair moves)."""
    if pairs:
        r = qp.quench_pairs(N, h, 0)
        return r["state"].astype(np.int64), int(r["energy_out"]), int(r["n_moves"]), int(r["n_pair_moves"])
    r = qu.quench(N, h)
    return r["state"].astype(np.int64), int(r["energy_out"]), int(r["n_moves"]), 0


def _search_host(N, h, pairs):
    import mcq_amd

    if pairs:
        r = mcq_amd.quench.quench_pairs_host(N, h.astype(np.uint8), conflicts=False)
        return r["state"][0].astype(np.int64), int(r["energy_out"][0]), int(r["n_moves"][0]), int(r["n_pair_moves"][0])
    r = mcq_amd.quench.quench_states_host(N, h.astype(np.uint8), conflicts=False)
    return r["state"][0].astype(np.int64), int(r["energy_out"][0]), int(r["n_moves"][0]), 0


def hop(N, board, seed, n_hops, kick=2, slack=0, local_search="pairs", first_hop=0, search="numpy"):
    """One board through the rule; returns a dict with the fields of mcq_hop plus `energy_hist`, `trace`, `drawn_twice` (hops whose
    kick drew some column more than once) and `redrawn` (hops whose kick drew some column twice with DIFFERENT heights: only there does
    the order of the draws show)."""
    L = {"numpy": _search_numpy, "host": _search_host}[search]
    pairs = {"single": False, "pairs": True}[local_search]
    h = qu.clamp(N, board).copy()
    e_in = qu.energy(N, h)
    h, E, moves, pair_moves = L(N, h, pairs)
    e_start = best = E
    best_hop, best_state = 0, h.copy()
    accepted = improved = 0
    hist, trace, twice, redrawn = [E], [], 0, 0
    for t in range(n_hops):
        before = h.copy()  # the copy a rejected hop is restored from
        draws = kick_draws(N, seed, first_hop + t, kick)
        twice += len({c for c, _ in draws}) < len(draws)
        redrawn += len({c for c, _ in draws}) < len(set(draws))  # some column with two heights
        for c, k in draws:
            h[c] = k
        h, e_new, m, p = L(N, h, pairs)
        moves, pair_moves = moves + m, pair_moves + p
        if e_new <= E + slack:
            accepted += 1
            E = e_new
            what = "same" if (h == before).all() else "changed"
            if E < best:
                best, best_hop, best_state = E, t + 1, h.copy()
                improved += 1
                what = "improved"
            trace.append(what)
        else:
            h = before
            trace.append("rejected")
        hist.append(E)
    return {"state": h.astype(np.uint8), "energy_in": e_in, "energy_start": e_start, "energy_out": E, "best_energy": best, "best_hop": best_hop,
            "best_state": best_state.astype(np.uint8), "n_accepted": accepted, "n_improved": improved, "n_moves": moves,
            "n_pair_moves": pair_moves, "energy_hist": np.array(hist, dtype=np.int64), "trace": trace, "drawn_twice": twice,
            "redrawn": redrawn, "kick": kick}


def hop_many(N, states, seeds, n_hops, **kw):
    rows = [hop(N, s, int(sd), n_hops, **kw) for s, sd in zip(np.asarray(states).reshape(-1, N * N), np.asarray(seeds).reshape(-1))]
    out = {k: np.stack([np.asarray(r[k]) for r in rows]) for k in FIELDS + ("energy_hist",)}
    out["trace"] = [r["trace"] for r in rows]
    out["drawn_twice"] = sum(r["drawn_twice"] for r in rows)
    out["redrawn"] = sum(r["redrawn"] for r in rows)
    out["kick"] = kw.get("kick", 2)
    return out


def assert_equal(got, want, what, hist=True):
    for k in FIELDS + (("energy_hist",) if hist else ()):
        np.testing.assert_array_equal(np.asarray(got[k]).astype(np.int64), np.asarray(want[k]).astype(np.int64), err_msg=f"{what}: {k}")


class Coverage:
    """The condition on the inputs: what the restatement's traces of a group of comparisons contain.  A group without rejected hops
    never ran the restore path, one without accepted hops on a changed placement never ran the commit path, and one whose kicks of three
    draws or more never draw a column twice with different heights never showed in which order the draws of a kick are applied."""

    def __init__(self):
        self.count = {}

    def add(self, group, want):
        c = self.count.setdefault(group, {"rejected": 0, "changed": 0, "improved": 0, "hops": 0, "redrawn": 0, "largest_kick": 0})
        c["redrawn"] += want["redrawn"]
        c["largest_kick"] = max(c["largest_kick"], want["kick"])
        for tr in want["trace"]:
            c["hops"] += len(tr)
            c["rejected"] += tr.count("rejected")
            c["changed"] += tr.count("changed") + tr.count("improved")
            c["improved"] += tr.count("improved")

    def check(self, group):
        c = self.count[group]
        assert c["rejected"] >= 3 and c["changed"] >= 3 and c["improved"] >= 1, (group, c)
        assert c["largest_kick"] < 3 or c["redrawn"] >= 1, (group, c)
        return c


MAX_KICK = 1024  # MCQ_MAX_HOP_KICK: more draws than any board has columns
MAX_KICK_CASES = ((4, 3, 8, ("single", "pairs")), (12, 2, 5, ("single", "pairs")), (32, 1, 3, ("pairs",)))  # N, chains, hops, local searches

_max_kick_cache = {}


def max_kick_case(N, search, accept_all):
    """(boards, seeds, hops, slack, the restated run) of the comparison with kick = MAX_KICK at N: every hop redraws nearly the whole board
    (64 draws per column at N = 4), once without slack and once with a slack above every energy.  The local search is the restatement's
    own at N = 4 and the library's quench host calls beyond.  Computed once per session, shared and left unchanged."""
    key = (N, search, accept_all)
    if key not in _max_kick_cache:
        import mcq_amd

        n, hops = next((c[1], c[2]) for c in MAX_KICK_CASES if c[0] == N)
        s = qu.random_boards(N, n, 9 + N, over=True)
        seeds = mcq_amd.abi.seeds_for(60 + N, n)
        slack = 4 * N * N * N if accept_all else 0  # E <= 4 (N - 1) N^2 / 2
        want = hop_many(N, s, seeds, hops, kick=MAX_KICK, slack=slack, local_search=search, search="numpy" if N == 4 else "host")
        _max_kick_cache[key] = (s, seeds, hops, slack, want)
    return _max_kick_cache[key]


def mark_first_hop(kick, before=2):
    """A first_hop `before` hops short of the hop whose kick holds word 2^35 of the stream: there w >> 34, the second counter word of the
    block of word w, goes from 1 to 2 (rule item 4: the high bits of w / 4)."""
    return (1 << 35) // (2 * kick) - before


def crosses_the_mark(kick, first_hop, n_hops):
    return (2 * kick * first_hop) >> 34 == 1 and (2 * kick * (first_hop + n_hops) - 1) >> 34 == 2


def merge(parts):
    """The figures of a run cut into the calls `parts` (in order, each fed the `state` of the one before and first_hop carried over), as
    hop_states' docstring says: n_accepted, n_moves and n_pair_moves add up, energy_in / energy_start are the first call's, state /
    energy_out the last call's, best_* those of the FIRST call with the smallest best_energy, its best_hop moved by the hops before that
    call; the histories are joined without the repeated first entry, and n_improved counts the new lows of the joined history (a
    call counts its improvements against its own start, so with slack > 0 they do not add up)."""
    out = {"state": parts[-1]["state"], "energy_out": parts[-1]["energy_out"], "energy_in": parts[0]["energy_in"], "energy_start": parts[0]["energy_start"]}
    for k in ("n_accepted", "n_moves", "n_pair_moves"):
        out[k] = sum(np.asarray(p[k]).astype(np.int64) for p in parts)
    be = np.stack([np.asarray(p["best_energy"]).astype(np.int64) for p in parts])
    first = be.argmin(axis=0)  # the first of the smallest
    n_hops = [p["energy_hist"].shape[1] - 1 for p in parts]
    before = np.concatenate([[0], np.cumsum(n_hops)[:-1]])
    rows = np.arange(be.shape[1])
    out["best_energy"] = be[first, rows]
    hop_in_call = np.stack([np.asarray(p["best_hop"]).astype(np.int64) for p in parts])[first, rows]
    # best_hop = 0 of a later call is the placement it was handed: the end of the call before, whose best_energy is no larger -- so the
    # first call with the smallest best_energy never has it, except the very first call
    out["best_hop"] = hop_in_call + before[first]
    out["best_state"] = np.stack([p["best_state"] for p in parts])[first, rows]
    out["energy_hist"] = np.concatenate([parts[0]["energy_hist"]] + [p["energy_hist"][:, 1:] for p in parts[1:]], axis=1)
    low = np.minimum.accumulate(out["energy_hist"].astype(np.int64), axis=1)
    out["n_improved"] = (low[:, 1:] < low[:, :-1]).sum(axis=1)
    return out
