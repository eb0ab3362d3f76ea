"""The tabu rule of include/mcq.h (mcq_tabu) restated in NumPy, from the text of the rule and from nothing else: a(c, k) is recounted
naively before every iteration, the stamps T(c, k) are absolute Python-sized integers in an int64 array, and every iteration leaves a
trace.  What mcq_tabu_host is compared with, and where the tests learn whether aspiration, the rotation of ties and the stall ran.
Below the rule: the inputs that sleep until iteration 2^15 of a call with the window that restates them, and the boards at the ends of
the kernel's packed key."""
import functools

import numpy as np

from tests import heatbath_util as hb
from tests import quench_util as qu

FIELDS = ("state", "energy_in", "energy_out", "best_energy", "best_iter", "best_state", "n_moves", "n_aspired", "n_uphill", "n_stalled",
          "energy_hist", "tabu_out")
COUNTERS = ("n_moves", "n_aspired", "n_uphill", "n_stalled")
KEY_WORD = 7


@functools.lru_cache(maxsize=None)
def _pairs(N):
    """Every ordered pair of aligned columns (c, c'), flat: (c, c', d = max(|di|, |dj|))."""
    ii, jj = (x.ravel() for x in np.indices((N, N)))
    di, dj = np.abs(ii[:, None] - ii[None, :]), np.abs(jj[:, None] - jj[None, :])
    on = ((di == 0) | (dj == 0) | (di == dj)) & ((di != 0) | (dj != 0))
    c, c2 = np.nonzero(on)
    return c, c2, np.maximum(di, dj)[on]


def table(N, h):
    """a(c, k) as int64[N*N][N], recounted from the heights: a queen at height h' in an aligned column at distance d attacks the heights
    h', h' - d and h' + d of column c."""
    c, c2, d = _pairs(N)
    a = np.zeros(N * N * N, dtype=np.int64)
    for s in (-1, 0, 1):
        k = h[c2] + s * d
        ok = (k >= 0) & (k < N)
        a += np.bincount((c * N + k)[ok], minlength=N * N * N)
    return a.reshape(N * N, N)


def draw(seed, g, N, tenure_rand):
    """(o, jitter) of iteration g."""
    x = hb.philox((g & hb.MASK, g >> 32, 0, 0), (seed, KEY_WORD))
    return (x[0] * N ** 3) >> 32, (x[1] * (tenure_rand + 1)) >> 32


def tabu(N, board, seed, n_iters, tenure=10, tenure_rand=0, tenure_conf=0, first_iter=0, tabu_in=None, best_floor=None):
    """One chain through the rule; returns a dict with the fields of mcq_tabu plus `trace`, one dict per iteration."""
    Q, N3 = N * N, N ** 3
    h = qu.clamp(N, board).copy()
    assert np.array_equal(table(N, h), qu.table(N, h)) if Q <= 36 else True  # the two recounts agree where the slow one is cheap
    T = np.zeros((Q, N), dtype=np.int64)
    if tabu_in is not None:
        T = first_iter + np.asarray(tabu_in, dtype=np.int64).reshape(Q, N)
    cols, ks = np.indices((Q, N))
    written = np.full((Q, N), -1, dtype=np.int64)  # the iteration whose move wrote T(c, k); -1: the stamp is the call's tabu_in
    a = table(N, h)
    e_in = int(a[np.arange(Q), h].sum()) // 2
    E = e_in
    B = e_in if best_floor is None else min(int(best_floor), e_in)
    best, best_iter = h.copy(), 0
    hist, trace = [E], []
    n = dict.fromkeys(COUNTERS, 0)
    for t in range(n_iters):
        g = first_iter + t
        o, jitter = draw(seed, g, N, tenure_rand)
        a = table(N, h)
        now = a[np.arange(Q), h]
        assert int(now.sum()) == 2 * E
        delta = a - now[:, None]
        cand = (now[:, None] > 0) & (ks != h[:, None])
        is_tabu = T > g
        adm = cand & (~is_tabu | (E + delta < B))
        F = int((now > 0).sum())
        held = cand & is_tabu & ~(E + delta < B) & (written >= 0)  # candidates that a stamp of an earlier move of this call keeps out
        tr = {"candidates": int(cand.sum()), "F": F, "E": E, "o": o, "moved": False, "g": g, "held_since": int(written[held].min()) if held.any() else None}
        if not adm.any():
            n["n_stalled"] += 1
        else:
            idx = cols * N + ks
            rho = (idx - o) % N3
            dmin = int(delta[adm].min())
            ties = adm & (delta == dmin)
            w = int(idx[ties][np.argmin(rho[ties])])
            c, k = divmod(w, N)
            L = tenure + jitter + (tenure_conf * F) // 16
            tr.update(moved=True, tabu=bool(is_tabu[c, k]), delta=dmin, not_first=w != int(idx[ties].min()), wrapped=w < o, L=L, ties=int(ties.sum()),
                      new_best=E + dmin < B)
            n["n_moves"] += 1
            n["n_aspired"] += int(is_tabu[c, k])
            n["n_uphill"] += int(dmin > 0)
            T[c, h[c]] = g + 1 + L
            written[c, h[c]] = g
            h[c] = k
            E += dmin
            if E < B:
                B, best_iter, best = E, t + 1, h.copy()
        hist.append(E)
        trace.append(tr)
    out = {"state": h.astype(np.uint8), "energy_in": e_in, "energy_out": E, "best_energy": B, "best_iter": best_iter, "best_state": best.astype(np.uint8),
           "energy_hist": np.array(hist, dtype=np.int64), "tabu_out": np.maximum(0, T - (first_iter + n_iters)).reshape(-1), "trace": trace}
    out.update(n)
    assert out["tabu_out"].max() < 1 << 16
    return out


def tabu_many(N, states, seeds, n_iters, tabu_in=None, best_floor=None, **kw):
    states = np.asarray(states).reshape(-1, N * N)
    rows = [tabu(N, s, int(seed), n_iters, tabu_in=None if tabu_in is None else np.asarray(tabu_in).reshape(len(states), -1)[r],
                 best_floor=None if best_floor is None else best_floor[r], **kw) for r, (s, seed) in enumerate(zip(states, seeds))]
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
    for k in ("state", "energy_out", "best_energy", "tabu_out"):
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
    """fn (tabu_host, tabu_states, tabu_many) over the pieces `cuts`, each fed the state, tabu_out and best_energy of the one before."""
    parts, state, ti, bf, done = [], s, tabu_in, best_floor, first_iter
    for iters in cuts:
        parts.append(fn(N, state, seeds, iters, first_iter=done, tabu_in=ti, best_floor=bf, **kw))
        state, ti, bf, done = parts[-1]["state"], parts[-1]["tabu_out"], parts[-1]["best_energy"], done + iters
    return parts


class Coverage:
    """What a group of compared runs must contain before the comparison counts: from the restatement's traces."""

    NEED = {"aspired": 3, "uphill": 3, "not_first": 3, "wrapped": 1, "stall_above_0": 1, "best_after_uphill": 1}

    def __init__(self):
        self.n = {}

    def add(self, group, traces):
        n = self.n.setdefault(group, dict.fromkeys(self.NEED, 0))
        for chain in traces:
            rose = False
            for tr in chain:
                if not tr["moved"]:
                    n["stall_above_0"] += tr["E"] > 0
                    continue
                n["aspired"] += tr["tabu"]
                n["uphill"] += tr["delta"] > 0
                n["not_first"] += tr["not_first"]
                n["wrapped"] += tr["wrapped"]
                rose = rose or tr["delta"] > 0
                if tr["new_best"] and rose:
                    n["best_after_uphill"] += 1
                    rose = False

    def check(self, group):
        n = self.n[group]
        for k, need in self.NEED.items():
            assert n[k] >= need, f"group {group}: {k} = {n[k]} < {need}: {n}"
        return n


def counters_cover(got):
    """The part of the coverage that the outputs themselves show, for runs too long for the restatement: aspired and uphill moves, a
    stall of a chain whose energy never reached 0, and a new best behind a rise of the history."""
    hist = np.asarray(got["energy_hist"]).astype(np.int64)
    low = np.minimum.accumulate(hist, axis=1)
    after = 0
    for r in range(hist.shape[0]):
        rises = np.flatnonzero(np.diff(hist[r]) > 0)
        news = np.flatnonzero(low[r, 1:] < low[r, :-1])
        after += bool(len(rises) and len(news) and news[-1] > rises[0])
    return {"aspired": int(got["n_aspired"].sum()), "uphill": int(got["n_uphill"].sum()),
            "stall_above_0": int(((got["n_stalled"] > 0) & (hist.min(axis=1) > 0)).sum()), "best_after_uphill": after}


# Inputs that sleep, then wake across the move of the kernel's stamp base.  With every entry of a chain tabu and best_floor = 0 the rule
# admits nothing: the chain stalls, and its placement and absolute stamps stay as they are until the first stamp expires.  So the run
# from iteration W on is, by consequence (b), the run with first_iter = W, tabu_in - W and best_floor = 0, and only that window has to
# be restated, while a kernel has to run all of it in one call and move its base at iteration REBASE of the call.
REBASE = 1 << 15
LONGEST = dict(tenure=8192, tenure_rand=4095, tenure_conf=64)
SLEEP_EXPIRIES = {"spread": (32700, 32841, 32700), "edge": (32767, 32771, 32760)}  # variant -> [low, high) of tabu_in, and W


def sleeping(N, n, seed, variant):
    """(tabu_in, W): n chains whose every entry is tabu until it expires around iteration 2^15 of the call, none before W.  "spread":
    expiries U[32700, 32840]; "edge": only 32767, 32768, 32769 and 32770, so everything wakes within three iterations of the move."""
    lo, hi, W = SLEEP_EXPIRIES[variant]
    return np.random.RandomState(seed).randint(lo, hi, size=(n, N ** 3)).astype(np.uint16), W


def wake(N, states, seeds, n_iters, tabu_in, W, **kw):
    """The outputs of the sleeping run of n_iters >= W iterations from iteration 0, restated over [W, n_iters) alone; `trace` holds the
    window (trace[r][i] is iteration W + i)."""
    n = len(states)
    win = tabu_many(N, states, seeds, n_iters - W, first_iter=W, tabu_in=np.asarray(tabu_in).astype(np.int64) - W, best_floor=np.zeros(n, dtype=np.int64), **kw)
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


def wake_cover(traces, mark=REBASE):
    """Of the windows' traces: moves before and from iteration `mark` on, and the iterations from `mark` on in which a stamp written
    before `mark` keeps a candidate out."""
    n = {"moves_before": 0, "moves_after": 0, "held_across": 0}
    for chain in traces:
        for tr in chain:
            n["moves_before"] += tr["moved"] and tr["g"] < mark
            n["moves_after"] += tr["moved"] and tr["g"] >= mark
            n["held_across"] += tr["g"] >= mark and tr["held_since"] is not None and tr["held_since"] < mark
    return n


# Boards at the ends of the kernel's packed key (delta + 124) << 15 | rho
def flat_board(N):
    """Every queen at height 0: each column is attacked by all its aligned columns, and the first moves take delta = -max a(c, k)."""
    return np.zeros((1, N * N), dtype=np.uint8)


def uphill_board(N):
    """(board, tabu_in): flat but for the centre column at height N / 2, and every entry tabu for 50 iterations except (centre, 0).
    Under best_floor = 0 the only admissible move puts the centre queen back among all its aligned columns: the largest rise."""
    b = flat_board(N)
    centre = (N // 2) * N + N // 2
    b[0, centre] = N // 2
    tin = np.full((1, N * N, N), 50, dtype=np.uint16)
    tin[0, centre, 0] = 0
    return b, tin.reshape(1, -1)
