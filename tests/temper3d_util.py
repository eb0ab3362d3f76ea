"""The full_3d tempering rule of include/mcq.h (mcq_temper3d) restated in NumPy and Python integers, from the text of the rule and from
nothing else.  Per slot it is tests/heatbath3d_util.sweeps (one sweep of one chain with the row of the slot's rung), the event is that
of tests/temper_util with key word 4, and a ladder with a repeated placement is held.  Naive on purpose (the counts of all cells are
rebuilt for every update): N <= 5."""
import numpy as np

from tests import heatbath3d_util as h3
from tests import heatbath_util as hu
from tests import quench3d_util as q3
from tests import temper_util as tu

MASK = hu.MASK
PER_SLOT = tu.PER_SLOT + ("flags",)
FIELDS = PER_SLOT + ("pair_accepted",)
REPEATED, HELD = 1, 2
tables = tu.tables
events = tu.events
check_invariants = tu.check_invariants


def exchange_word(seed0, w):
    """Word w (a Python integer) of the exchange stream of a ladder whose slot 0 is seeded seed0: key word 4."""
    b = w >> 2
    return hu.philox((b & MASK, b >> 32, 0, 0), (seed0, 4))[w & 3]


def ladder_run(N, placements, seeds, T, X, K, first_sweep=0, rungs=None, n_sweeps=None):
    """One ladder through the rule: placements [R][3 Q], seeds [R], T [n_sweeps][R][D], X [n_events][R - 1][DX].  Returns a dict with the
    fields of mcq_temper3d (arrays over the R slots; pair_accepted [R - 1]), energy_hist, rung_hist and `draws`, the (event e, pair t,
    Delta, x or None, swapped) of every pair looked at."""
    R, DX = len(seeds), X.shape[2]
    n_sweeps = T.shape[0] if n_sweeps is None else n_sweeps  # (no sweep: T holds one row that no sweep reads)
    rung = list(range(R)) if rungs is None else [int(t) for t in rungs]
    assert sorted(rung) == list(range(R))
    z = [q3.clamp(N, p) for p in placements]
    state = [c.astype(np.uint8).reshape(-1) for c in z]
    E = [q3.energy(N, c) for c in z]
    repeats = [bool(q3.is_repeated(N, c)) for c in z]
    if any(repeats):  # rule item 4: the whole ladder is handed back unmoved
        zero = np.zeros(R, dtype=np.int64)
        return {"state": np.stack(state), "energy_in": np.array(E), "energy_out": np.array(E), "best_energy": np.array(E), "best_sweep": zero,
                "best_state": np.stack(state), "n_changed": zero, "rung_out": np.array(rung), "n_exchanges": zero,
                "flags": np.array([HELD | (REPEATED if r else 0) for r in repeats]), "pair_accepted": np.zeros(R - 1, dtype=np.int64),
                "energy_hist": np.repeat(np.array(E, dtype=np.int32)[:, None], n_sweeps + 1, axis=1),
                "rung_hist": np.repeat(np.array(rung)[:, None], n_sweeps + 1, axis=1), "draws": []}
    e_in, best, best_sweep, best_state = list(E), list(E), [0] * R, [s.copy() for s in state]
    changed, exchanges, accepted = [0] * R, [0] * R, [0] * (R - 1)
    ehist, rhist, draws = [[e] for e in E], [[t] for t in rung], []
    for s in range(n_sweeps):
        g = first_sweep + s
        for r in range(R):
            one = h3.sweeps(N, state[r], int(seeds[r]), T[s: s + 1, rung[r]], 1, first_sweep=g)
            assert one["energy_in"] == E[r]
            state[r], E[r] = one["state"], one["energy_out"]
            changed[r] += one["n_changed"]
            ehist[r].append(E[r])
            if E[r] < best[r]:
                best[r], best_sweep[r], best_state[r] = E[r], s + 1, state[r].copy()
        if (g + 1) % K == 0:
            e = (g + 1) // K - 1
            j = e - first_sweep // K
            by_rung = {rung[r]: r for r in range(R)}
            for t in range(e % 2, R - 1, 2):
                a, b = by_rung[t], by_rung[t + 1]
                delta, x = E[b] - E[a], None
                if delta >= 0:
                    swap = True
                else:
                    x = exchange_word(int(seeds[0]), e * R + t)
                    swap = x < int(X[j, t, min(-delta, DX - 1)])
                draws.append((e, t, delta, x, swap))
                if swap:
                    rung[a], rung[b] = t + 1, t
                    exchanges[a] += 1
                    exchanges[b] += 1
                    accepted[t] += 1
        for r in range(R):
            rhist[r].append(rung[r])
    return {"state": np.stack(state).astype(np.uint8), "energy_in": np.array(e_in), "energy_out": np.array(E), "best_energy": np.array(best),
            "best_sweep": np.array(best_sweep), "best_state": np.stack(best_state).astype(np.uint8), "n_changed": np.array(changed),
            "rung_out": np.array(rung), "n_exchanges": np.array(exchanges), "flags": np.zeros(R, dtype=np.int64),
            "pair_accepted": np.array(accepted), "energy_hist": np.array(ehist, dtype=np.int32), "rung_hist": np.array(rhist), "draws": draws}


def run_many(N, states, seeds, betas, ladder, Q=None, K=1, first_sweep=0, rungs=None):
    """Every ladder of `states` through ladder_run; the arrays joined over the slots (pair_accepted: stacked over the ladders)."""
    R = len(ladder)
    Q = N * N if Q is None else Q
    T, X = tables(betas, ladder, K, first_sweep)
    states = np.asarray(states).reshape(-1, 3 * Q)
    outs = [ladder_run(N, states[g: g + R], seeds[g: g + R], T, X, K, first_sweep, None if rungs is None else rungs[g: g + R], len(betas))
            for g in range(0, len(states), R)]
    res = {k: np.concatenate([o[k] for o in outs]) for k in PER_SLOT + ("energy_hist", "rung_hist")}
    res["pair_accepted"] = np.stack([o["pair_accepted"] for o in outs])
    res["draws"] = [o["draws"] for o in outs]
    return res


def assert_equal(got, want, what, hist=False, fields=FIELDS):
    for k in tuple(fields) + (("energy_hist", "rung_hist") if hist else ()):
        g, w = np.asarray(got[k]).astype(np.int64), np.asarray(want[k]).astype(np.int64)
        np.testing.assert_array_equal(g.reshape(w.shape), w, err_msg=f"{what}: {k}")


def host_call(N, Q, s, seeds, T, X, K, first, rungs=None):
    """mcq_temper3d_host with the caller's own tables (T [n_sweeps][R][D], X [n_events][R - 1][DX]); returns the traced result dict."""
    import mcq_amd

    n, R, n_sweeps = s.shape[0], T.shape[1], T.shape[0]
    q = mcq_amd.tempering._block3d(N, Q, n, n_sweeps, first, R, K, T.shape[2], X.shape[2])
    out = mcq_amd.quench._host_outputs(q, s, mcq_amd.abi.TEMPER3D_DTYPES, like=("best_state",))
    out["pair_accepted"] = np.zeros((n // R, R - 1), dtype=np.int64)
    out["energy_hist"], out["rung_hist"] = np.zeros((n, n_sweeps + 1), dtype=np.int32), np.zeros((n, n_sweeps + 1), dtype=np.uint8)
    sd = np.ascontiguousarray(seeds, dtype=np.uint32)
    q.seeds, q.table, q.swap_table, q.pair_accepted = sd.ctypes.data, T.ctypes.data, X.ctypes.data, out["pair_accepted"].ctypes.data
    q.energy_hist, q.rung_hist, q.hist_stride = out["energy_hist"].ctypes.data, out["rung_hist"].ctypes.data, n_sweeps + 1
    if rungs is not None:
        q.rung_in = rungs.ctypes.data
    mcq_amd._lib.temper3d_host(q)
    return out


def fits(N, R, Q=None, D=512):
    """Whether mcq_temper3d_device runs the ladder, from the layout include/mcq.h states: per chain 72 dwords, the field (a byte per cell
    to N = 19, 16 bits beyond), the occupancy bits and 16 bits per queen, rounded up to 4 dwords; R D dwords of rows; 3 R words; and 256
    bytes of static LDS, within 160 KiB."""
    Q = N * N if Q is None else Q
    C = N ** 3
    fw = (C + 3) // 4 if N <= 19 else (C + 1) // 2
    chain = (72 + fw + (C + 31) // 32 + (Q + 1) // 2 + 3) // 4 * 4
    return 4 * (R * chain + R * D + 3 * R) + 256 <= 160 * 1024
