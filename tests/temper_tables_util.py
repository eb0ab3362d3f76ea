"""Weight and swap tables a CALLER may hand to the tempering entry points, which abi.temper_tables never builds (its weight rows start
at 2^24, fall monotonically and are zero from the first zero on; its swap rows start at 2^32 - 1 and do the same, alike for every pair
and nearly alike for every event), and what the tests of those tables share: the swap decision read back from the two histories under
a predicate of Delta, the closed form of the rungs under a table with which every pair swaps, and the kernels on a caller's tables."""
import functools

import numpy as np

from tests import temper3d_util as t3
from tests import temper_util as tu

M = 2**32 - 1
HIST = ("energy_hist", "rung_hist")
FAMILIES = ("zero3", "ones", "clip", "only1", "only3", "nonmono", "rand", "altzero")  # of tests/heatbath_tables_util.py: tables
SWAPS = ("zeros1", "zeros3", "max1", "only1", "clip", "ramp", "rand")
# which Delta of a looked-at pair swaps under the swap tables whose rows hold 0 and M only (M: unless the pair's word is M itself)
PREDICATES = {"zeros1": lambda d: d >= 0, "zeros3": lambda d: d >= 0, "only1": lambda d: d >= 0 or d == -1, "clip": lambda d: d >= 0 or d <= -2}


def _padded(rows, D):
    """uint32[n][d] as uint32[n][D], each row's last entry repeated: a distance beyond d - 1 reads the last entry either way."""
    rows = np.asarray(rows, dtype=np.uint32)
    return np.concatenate([rows, np.repeat(rows[:, -1:], D - rows.shape[1], axis=1)], axis=1)


def ladder_tables(n_sweeps, R):
    """{name: uint32[n_sweeps][R][D]} from the families of heatbath_tables_util.tables:
    same:<family>  the family's row of the sweep on every rung
    mixed          rung t of sweep s takes the row of family (s + t) mod 8, each padded to the longest D with its last entry
    mixed_full     rung 0 all 2^24 at D = 512 (the largest W the bound allows), the other rungs from `mixed`, padded to 512"""
    from tests import heatbath_tables_util as ht

    fam = ht.tables(n_sweeps)
    D = max(fam[f].shape[1] for f in FAMILIES)
    out = {f"same:{f}": np.ascontiguousarray(np.repeat(fam[f][:, None, :], R, axis=1)) for f in FAMILIES}
    mixed = np.zeros((n_sweeps, R, D), dtype=np.uint32)
    for s in range(n_sweeps):
        for t in range(R):
            mixed[s, t] = _padded(fam[FAMILIES[(s + t) % len(FAMILIES)]][s: s + 1], D)[0]
    out["mixed"] = mixed
    full = np.stack([_padded(mixed[s], fam["full"].shape[1]) for s in range(n_sweeps)]) if n_sweeps else np.zeros((0, R, fam["full"].shape[1]), dtype=np.uint32)
    full[:, 0, :] = ht.B
    out["mixed_full"] = np.ascontiguousarray(full)
    assert all(v.dtype == np.uint32 and v.shape[:2] == (n_sweeps, R) and v.flags.c_contiguous and int(v.max(initial=0)) <= ht.B for v in out.values())
    return out


def swap_tables(n_events, R, seed):
    """{name: uint32[n_events][R - 1][DX]}, M = 2^32 - 1, and when a looked-at pair with Delta < 0 swaps:
    zeros1, zeros3  DX = 1 and 3, all 0: never
    max1            DX = 1, all M: always, unless its word is M
    only1           [0, M, 0]: at Delta = -1
    clip            [0, 0, M]: at Delta <= -2, the clamp to DX - 1 landing on a live entry
    ramp            DX = 4096, X[d] = d 2^20: it RISES, so a read one entry off changes the decision
    rand            DX = 5, RandomState(seed) over the full 32 bits, another row for every event and every pair"""
    def rep(row):
        return np.ascontiguousarray(np.tile(np.array(row, dtype=np.uint32), (n_events, R - 1, 1)))

    t = {"zeros1": rep([0]), "zeros3": rep([0, 0, 0]), "max1": rep([M]), "only1": rep([0, M, 0]), "clip": rep([0, 0, M]),
         "ramp": rep(np.arange(4096, dtype=np.uint64) << 20),
         "rand": np.random.RandomState(seed).randint(0, 2**32, size=(n_events, R - 1, 5), dtype=np.uint64).astype(np.uint32)}
    assert tuple(t) == SWAPS and all(v.dtype == np.uint32 and v.shape[:2] == (n_events, R - 1) and v.flags.c_contiguous for v in t.values())
    return t


def aimed(seed0, R, first_event, n_events, key_word, bump):
    """uint32[n_events][R - 1][4]: every entry of row (j, t) is the word x that pair t of event first_event + j draws, plus bump.
    With bump = 0 `x < X[..]` fails by one and nothing swaps below Delta = 0 (the run under zeros1); with bump = 1 it holds by one and
    every looked-at pair swaps (the run under max1).  The words are those of a ladder whose slot 0 is seeded seed0: the caller gives
    every ladder of the call that seed."""
    word = {3: tu.exchange_word, 4: t3.exchange_word}[key_word]
    assert bump in (0, 1)
    X = np.zeros((n_events, R - 1, 4), dtype=np.uint32)
    for j in range(n_events):
        for t in range(R - 1):
            x = word(int(seed0), (first_event + j) * R + t)
            assert x != M, "the word is 2^32 - 1: no entry lies above it"
            X[j, t] = x + bump
    return X


def assert_swaps_follow(got, R, K, first, pred):
    """From energy_hist and rung_hist of a traced result (every ladder): each pair an event looks at -- the pairs of its parity, the
    energies by rung as the sweep before it left them -- swapped exactly when pred(Delta) holds.  Returns the number of looked-at pairs
    with Delta >= 0, Delta = -1 and Delta <= -2."""
    rh, eh = np.asarray(got["rung_hist"]).astype(np.int64), np.asarray(got["energy_hist"]).astype(np.int64)
    n, T1 = rh.shape
    L = n // R
    rh, eh = rh.reshape(L, R, T1), eh.reshape(L, R, T1)
    counts = [0, 0, 0]
    for s in range(T1 - 1):
        g = first + s
        if (g + 1) % K:
            continue
        e = (g + 1) // K - 1
        before, after = rh[:, :, s], rh[:, :, s + 1]
        E = np.take_along_axis(eh[:, :, s + 1], np.argsort(before, axis=1), axis=1)  # energies by rung, before the event
        for t in range(e % 2, R - 1, 2):
            swapped = ((after == before + 1) & (before == t)).any(axis=1)
            delta = E[:, t + 1] - E[:, t]
            np.testing.assert_array_equal(swapped, np.array([bool(pred(int(d))) for d in delta]), err_msg=f"event {e} pair {t}, Delta {delta}")
            counts[0] += int((delta >= 0).sum())
            counts[1] += int((delta == -1).sum())
            counts[2] += int((delta <= -2).sum())
    return tuple(counts)


def transposition_rungs(R, rung_in, first, n_sweeps, K):
    """int64[n][n_sweeps + 1]: the rung of every slot after every sweep when each pair of the parity e mod 2 swaps at event e, whatever
    the energies: odd-even transposition.  rung_in is uint8[n] (a permutation per ladder) or None (slot r on rung r mod R)."""
    rung = np.asarray(rung_in).astype(np.int64).copy()
    hist = [rung.copy()]
    for s in range(n_sweeps):
        g = first + s
        if (g + 1) % K == 0:
            e = (g + 1) // K - 1
            low = (rung % 2 == e % 2) & (rung + 1 < R)          # the lower rung of a pair of the event's parity: up
            high = (rung % 2 != e % 2) & (rung >= 1)            # the upper rung of such a pair: down
            rung = rung + low - high
        hist.append(rung.copy())
    return np.stack(hist, axis=1)


def device_tables(T, X, dev):
    """The caller's tables on the device as temper_device takes them: int32 tensors, the uint32 entries bit for bit."""
    import torch

    return torch.from_numpy(np.ascontiguousarray(T).view(np.int32)).to(dev), torch.from_numpy(np.ascontiguousarray(X).view(np.int32)).to(dev)


def own_tables(N, s, seeds, T, X, K, first, rungs=None, form="counters", Q=None):
    """temper_device -- temper_queens_device when Q is given -- with the caller's own tables, traced, as NumPy arrays.  T and X are NumPy
    uint32 arrays or the int32 device tensors of device_tables; `rungs` may be a device tensor too."""
    import torch

    import mcq_amd

    tempering = mcq_amd.tempering
    dev = torch.device("cuda", torch.cuda.current_device())
    tabs = (T, X) if isinstance(T, torch.Tensor) else device_tables(T, X, dev)
    kw = dict(tables=tabs, exchange_every=K, first_sweep=first, rungs=rungs, trace=True)
    if Q is None:
        res = tempering.temper_device(N, torch.from_numpy(s).to(dev), seeds, form=form, **kw)
    else:
        res = tempering.temper_queens_device(N, torch.from_numpy(s).to(dev), seeds, Q=Q, **kw)
    torch.cuda.current_stream(dev).synchronize()
    return tempering.to_numpy(res)


def placements(kind, N, Q, n, seed):
    """uint8[n][N*N] boards (kind "board") or uint8[n][3 Q] full_3d placements (kind "cube"); an odd seed gives bytes >= N, which are clamped."""
    from tests import quench3d_util as q3
    from tests import quench_util as qu

    return qu.random_boards(N, n, seed, over=seed % 2 == 1) if kind == "board" else q3.random_placements(N, n, seed, Q=Q, over=seed % 2 == 1).reshape(n, 3 * Q)


def rungs(n, R, seed):
    rs = np.random.RandomState(seed)
    return np.concatenate([rs.permutation(R) for _ in range(n // R)]).astype(np.uint8)


WORD_FIRST, WORD_SWEEPS, WORD_R = 2**30 - 3, 6, 16  # K = 1: the events 2^30 - 3 .. 2^30 + 2, and e R + t crosses 2^34 at e = 2^30


@functools.lru_cache(maxsize=None)
def word_case(kind, N, Q, ladders=3):
    """(s, seeds, T, X, rungs): the inputs of the word-index case, shared with tests/test_temper_tables.py and left unchanged."""
    import mcq_amd

    n = WORD_R * ladders
    s, seeds = placements(kind, N, Q, n, 9 + N), mcq_amd.abi.seeds_for(4100000000 + N, n)
    T = mcq_amd.abi.temper_tables(np.linspace(0.6, 1.6, WORD_SWEEPS), [float(l) for l in np.linspace(0.5, 2.0, WORD_R)], 1, WORD_FIRST)[0]
    return s, seeds, T, swap_tables(WORD_SWEEPS, WORD_R, N)["rand"], rungs(n, WORD_R, N)


def word_sides(want):
    """From a traced result of the word-index case: the looked-at pairs with Delta < 0 (each draws a word) below and from 2^34 on."""
    sides = [0, 0]
    rh, eh = want["rung_hist"].astype(np.int64), want["energy_hist"].astype(np.int64)
    L = rh.shape[0] // WORD_R
    rh, eh = rh.reshape(L, WORD_R, -1), eh.reshape(L, WORD_R, -1)
    for s in range(WORD_SWEEPS):
        e = WORD_FIRST + s
        E = np.take_along_axis(eh[:, :, s + 1], np.argsort(rh[:, :, s], axis=1), axis=1)
        for t in range(e % 2, WORD_R - 1, 2):
            sides[e * WORD_R + t >= 2**34] += int((E[:, t + 1] - E[:, t] < 0).sum())
    return tuple(sides)


def assert_cut_equals_whole(a, b, whole, cut, what):
    """Two calls, the second from the first's state and rungs, against the unbroken call: every output and both histories."""
    for k in ("state", "energy_out", "rung_out"):
        np.testing.assert_array_equal(np.asarray(b[k]).reshape(np.asarray(whole[k]).shape), whole[k], err_msg=f"{what}: {k}")
    np.testing.assert_array_equal(a["energy_in"], whole["energy_in"], err_msg=what)
    np.testing.assert_array_equal(b["energy_in"], a["energy_out"], err_msg=what)
    for k in HIST:
        np.testing.assert_array_equal(np.concatenate([a[k], b[k][:, 1:]], axis=1), whole[k], err_msg=f"{what}: {k}")
    for k in ("n_changed", "n_exchanges", "pair_accepted"):
        np.testing.assert_array_equal(a[k] + b[k], whole[k], err_msg=f"{what}: {k}")
    later = b["best_energy"] < a["best_energy"]
    np.testing.assert_array_equal(np.where(later, b["best_energy"], a["best_energy"]), whole["best_energy"], err_msg=what)
    np.testing.assert_array_equal(np.where(later, b["best_sweep"] + cut, a["best_sweep"]), whole["best_sweep"], err_msg=what)
    w = np.asarray(whole["best_state"])
    np.testing.assert_array_equal(np.where(later[:, None], np.asarray(b["best_state"]).reshape(w.shape), np.asarray(a["best_state"]).reshape(w.shape)), w, err_msg=what)
