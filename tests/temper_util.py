"""The tempering rule of include/mcq.h (mcq_temper) restated in NumPy and Python integers, from the text of the rule and from nothing
else.  It builds on tests/heatbath_util.py: `philox`, `sweeps` (one sweep of one chain with a given row) and `table`."""
import numpy as np

from tests import heatbath_util as hu

MASK = hu.MASK
PER_SLOT = ("state", "energy_in", "energy_out", "best_energy", "best_sweep", "best_state", "n_changed", "rung_out", "n_exchanges")
FIELDS = PER_SLOT + ("pair_accepted",)


def exchange_word(seed0, w):
    """Word w (a Python integer) of the exchange stream of a ladder whose slot 0 is seeded seed0: key word 3."""
    b = w >> 2
    return hu.philox((b & MASK, b >> 32, 0, 0), (seed0, 3))[w & 3]


def events(first_sweep, n_sweeps, K):
    return (first_sweep + n_sweeps) // K - first_sweep // K


def tables(betas, ladder, K=1, first_sweep=0):
    """T[s][t][d] = floor(2^24 exp(-beta_s l_t d)) and X[j][t][d] = min(2^32 - 1, floor(2^32 exp(-beta_g (l_{t+1} - l_t) d))), g the
    sweep event j follows; each as long as its last row needs for its first zero (T: at most 512; X: at most 4096), rows of exponent 0
    being constant."""
    R = len(ladder)
    prod = [np.float64(b) * np.float64(l) for b in betas for l in ladder]
    T = hu.table(prod)
    T = T.reshape(len(betas), R, -1) if len(betas) else np.repeat(T.reshape(1, 1, 1), R, axis=1)
    rows, longest = [], 1
    for j in range(events(first_sweep, len(betas), K)):
        g = (first_sweep // K + 1 + j) * K - 1
        pairs = []
        for t in range(R - 1):
            x = np.float64(betas[g - first_sweep]) * (np.float64(ladder[t + 1]) - np.float64(ladder[t]))
            if x == 0:
                pairs.append(None)
                continue
            row = []
            for d in range(4096):
                v = min(2**32 - 1, int(np.floor(np.float64(2.0**32) * np.exp(-x * np.float64(d)))))
                row.append(v)
                if v == 0:
                    break
            assert row[-1] == 0, "the ladder step is too small for a table of 4096 entries"
            longest = max(longest, len(row))
            pairs.append(row)
        rows.append(pairs)
    X = np.zeros((len(rows), R - 1, longest), dtype=np.uint32)
    for j, pairs in enumerate(rows):
        for t, row in enumerate(pairs):
            X[j, t] = 2**32 - 1 if row is None else (row + [0] * longest)[:longest]
    return T, X


def ladder_run(N, boards, seeds, T, X, K, first_sweep=0, rungs=None, n_sweeps=None):
    """One ladder through the rule: boards [R][N*N], seeds [R], T [n_sweeps][R][D], X [n_events][R - 1][DX].  Returns a dict with the
    fields of mcq_temper (arrays over the R slots; pair_accepted [R - 1]), energy_hist, rung_hist and `draws`, the (event e, pair t,
    Delta, x or None, swapped) of every pair looked at."""
    R, DX = len(seeds), X.shape[2]
    n_sweeps = T.shape[0] if n_sweeps is None else n_sweeps  # (no sweep: T holds one row that no sweep reads)
    rung = list(range(R)) if rungs is None else [int(t) for t in rungs]
    assert sorted(rung) == list(range(R))
    state = [np.asarray(b) for b in boards]
    first = [hu.sweeps(N, state[r], int(seeds[r]), T[:0, 0], 0) for r in range(R)]  # the recount of the clamped input
    state = [f["state"] for f in first]
    E = [f["energy_in"] for f in first]
    e_in, best, best_sweep, best_state = list(E), list(E), [0] * R, [s.copy() for s in state]
    changed, exchanges, accepted = [0] * R, [0] * R, [0] * (R - 1)
    ehist, rhist, draws = [[e] for e in E], [[t] for t in rung], []
    for s in range(n_sweeps):
        g = first_sweep + s
        for r in range(R):
            one = hu.sweeps(N, state[r], int(seeds[r]), T[s: s + 1, rung[r]], 1, first_sweep=g)
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
            "rung_out": np.array(rung), "n_exchanges": np.array(exchanges), "pair_accepted": np.array(accepted),
            "energy_hist": np.array(ehist, dtype=np.int32), "rung_hist": np.array(rhist), "draws": draws}


def run_many(N, states, seeds, betas, ladder, K=1, first_sweep=0, rungs=None):
    """Every ladder of `states` through ladder_run; the arrays joined over the slots (pair_accepted: stacked over the ladders)."""
    R = len(ladder)
    T, X = tables(betas, ladder, K, first_sweep)
    states = np.asarray(states).reshape(-1, N * N)
    outs = [ladder_run(N, states[g: g + R], seeds[g: g + R], T, X, K, first_sweep, None if rungs is None else rungs[g: g + R], len(betas))
            for g in range(0, len(states), R)]
    res = {k: np.concatenate([o[k] for o in outs]) for k in PER_SLOT + ("energy_hist", "rung_hist")}
    res["pair_accepted"] = np.stack([o["pair_accepted"] for o in outs])
    res["draws"] = [o["draws"] for o in outs]
    return res


def assert_equal(got, want, what, hist=False, fields=FIELDS):
    for k in tuple(fields) + (("energy_hist", "rung_hist") if hist else ()):
        np.testing.assert_array_equal(np.asarray(got[k]).astype(np.int64), np.asarray(want[k]).astype(np.int64), err_msg=f"{what}: {k}")


def host_call(N, s, seeds, T, X, K, first, rungs=None):
    """mcq_temper_host with the caller's own tables (T [n_sweeps][R][D], X [n_events][R - 1][DX]); returns the traced result dict."""
    import mcq_amd

    n, R, n_sweeps = s.shape[0], T.shape[1], T.shape[0]
    q = mcq_amd.tempering._block(N, n, n_sweeps, first, R, K, T.shape[2], X.shape[2])
    out = mcq_amd.quench._host_outputs(q, s, mcq_amd.abi.TEMPER_DTYPES, like=("best_state",))
    out["pair_accepted"] = np.zeros((n // R, R - 1), dtype=np.int64)
    out["energy_hist"], out["rung_hist"] = np.zeros((n, n_sweeps + 1), dtype=np.int32), np.zeros((n, n_sweeps + 1), dtype=np.uint8)
    sd = np.ascontiguousarray(seeds, dtype=np.uint32)
    q.seeds, q.table, q.swap_table, q.pair_accepted = sd.ctypes.data, T.ctypes.data, X.ctypes.data, out["pair_accepted"].ctypes.data
    q.energy_hist, q.rung_hist, q.hist_stride = out["energy_hist"].ctypes.data, out["rung_hist"].ctypes.data, n_sweeps + 1
    if rungs is not None:
        q.rung_in = rungs.ctypes.data
    mcq_amd._lib.temper_host(q)
    return out


def check_invariants(got, R, K, first, swap_zero=False):
    """The exchange's invariants on a traced result (every ladder): rungs a permutation after every sweep; sum of n_exchanges =
    2 sum of pair_accepted; an event moves only pairs of its parity, by one rung; without an event nothing moves; and with a swap
    table of zeros a pair swaps exactly when Delta >= 0."""
    rh, eh = got["rung_hist"].astype(np.int64), got["energy_hist"].astype(np.int64)
    n, T1 = rh.shape
    L = n // R
    rh, eh = rh.reshape(L, R, T1), eh.reshape(L, R, T1)
    assert (np.sort(rh, axis=1) == np.arange(R)[None, :, None]).all(), "the rungs of a ladder are no permutation"
    np.testing.assert_array_equal(got["rung_out"].reshape(L, R), rh[:, :, -1])
    np.testing.assert_array_equal(got["n_exchanges"].reshape(L, R).sum(axis=1), 2 * got["pair_accepted"].sum(axis=1))
    np.testing.assert_array_equal(got["n_exchanges"].reshape(L, R), (rh[:, :, 1:] != rh[:, :, :-1]).sum(axis=2))
    pairs = np.zeros_like(got["pair_accepted"])
    for s in range(T1 - 1):
        g = first + s
        before, after = rh[:, :, s], rh[:, :, s + 1]
        if (g + 1) % K:
            assert (before == after).all(), f"sweep {s}: a rung moved without an event"
            continue
        e = (g + 1) // K - 1
        up, down = after == before + 1, after == before - 1
        assert (up | down | (after == before)).all()
        assert ((before[up] % 2) == e % 2).all() and ((after[down] % 2) == e % 2).all(), f"event {e} moved a pair of the other parity"
        for t in range(R - 1):
            pairs[:, t] += (up & (before == t)).sum(axis=1)
        if swap_zero:
            E = np.take_along_axis(eh[:, :, s + 1], np.argsort(before, axis=1), axis=1)  # energies by rung, before the event
            for t in range(e % 2, R - 1, 2):
                swapped = (up & (before == t)).any(axis=1)
                np.testing.assert_array_equal(swapped, E[:, t + 1] - E[:, t] >= 0, err_msg=f"event {e} pair {t}")
    np.testing.assert_array_equal(pairs, got["pair_accepted"])
