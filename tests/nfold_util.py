"""The n-fold rule of include/mcq.h (mcq_nfold) restated in NumPy and Python integers, from the text of the rule and from nothing else:
what mcq_nfold_host and the kernel are compared with.  Philox is this file's own, the 128-bit product is a Python integer, and a(c, k)
is that of tests/quench_util.py."""
import numpy as np

from tests import quench_util as qu

MASK = 0xFFFFFFFF
KEY_WORD = 11
TIME_BITS = 12
FIELDS = ("state", "best_state", "energy_in", "energy_out", "best_energy", "best_step", "events_out", "n_uphill", "n_flat", "need_out", "weight_out")


def philox(ctr, key):
    """philox4x32-10 on Python integers: (4 counter words, 2 key words) -> 4 output words."""
    c0, c1, c2, c3 = (int(v) for v in ctr)
    k0, k1 = (int(v) for v in key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + 0x9E3779B9) & MASK, (k1 + 0xBB67AE85) & MASK
    return [c0, c1, c2, c3]


def block(seed, e):
    """Block e of the chain seeded `seed` (rule item 5)."""
    return philox((e & MASK, e >> 32, 0, 0), (int(seed), KEY_WORD))


def ell(x, ln2, clock_table):
    """l(x) = z clock_ln2 + clock_table[y]: z leading zero bits, y the 8 bits below the leading one bit (zeros where there are none)."""
    x = int(x)
    if x == 0:
        return 32 * int(ln2) + int(clock_table[0])
    z = 32 - x.bit_length()
    y = (((x << z) & MASK) >> 23) & 255
    return z * int(ln2) + int(clock_table[y])


def weights(N, h, row):
    """w(c, k) as an int64 array [N*N][N] of the clamped heights h under the weight row `row`; 0 at k = h(c)."""
    t = qu.table(N, h)
    cols = np.arange(N * N)
    d = t - t[cols, h][:, None]
    w = np.asarray(row, dtype=np.int64)[np.clip(d, 0, len(row) - 1)]
    w[cols, h] = 0
    return w, d


def nfold(N, board, seed, tables, seg_steps, clock, first_seg=0, need_in=None, events_in=0, trace=None):
    """One board through the rule; returns a dict with the fields of mcq_nfold plus `energy_hist`.  `trace` (a list) receives
    (segment, left, c, k, d, U, W, lo, hi, zero_before) of every event: the chosen move holds the integers lo <= U < hi of 0 .. W - 1,
    and zero_before says whether the move before it in walk order (c ascending, k ascending, k = h(c) skipped) has weight 0."""
    ln2, ct = clock
    h = qu.clamp(N, board).copy()
    Q, M = N * N, N * N * (N - 1)
    E = qu.energy(N, h)
    e = int(events_in)
    x = block(seed, e)
    need = int(need_in) if need_in is not None else M * ell(x[2], ln2, ct)
    e_in, best_e, best_step, best = E, E, 0, h.copy()
    up = flat = 0
    W = 0
    hist = [E]
    for s, row in enumerate(np.asarray(tables)):
        whole = int(seg_steps) << TIME_BITS
        left = whole
        while True:
            w, d = weights(N, h, row)
            R = w.sum(axis=1)
            assert int(R.max()) < 2**32
            W = int(R.sum())
            if W == 0:
                break
            tau = max(1, (need << TIME_BITS) // W)
            if tau > left:
                assert left * W < 2**64
                need -= (left * W) >> TIME_BITS
                assert need >= 0
                break
            left -= tau
            U = (((x[0] << 32) | x[1]) * W) >> 64
            sums = np.cumsum(w.reshape(-1))
            flat_index = int(np.searchsorted(sums, U, side="right"))  # the first inclusive prefix sum above U
            c, k = divmod(flat_index, N)
            assert k != h[c] and w[c, k] > 0
            dd = int(d[c, k])
            if trace is not None:
                before = flat_index - 1
                while before >= 0 and before % N == h[before // N]:
                    before -= 1
                trace_tail = (U, W, int(sums[flat_index]) - int(w[c, k]), int(sums[flat_index]), bool(before >= 0 and w.reshape(-1)[before] == 0))
            h[c] = k
            E += dd
            up += dd > 0
            flat += dd == 0
            e += 1
            if trace is not None:
                trace.append((s, left, c, k, dd) + trace_tail)
            if E < best_e:
                best_e, best_step, best = E, s * int(seg_steps) + ((whole - left) >> TIME_BITS), h.copy()
            x = block(seed, e)
            need = M * ell(x[2], ln2, ct)
        hist.append(E)
    assert E == qu.energy(N, h)
    return {"state": h.astype(np.uint8), "best_state": best.astype(np.uint8), "energy_in": e_in, "energy_out": E, "best_energy": best_e,
            "best_step": best_step, "events_out": e, "n_uphill": up, "n_flat": flat, "need_out": need, "weight_out": W if len(tables) else 0,
            "energy_hist": np.array(hist, dtype=np.int64)}


def _trace_of(traces):
    traces.append([])
    return traces[-1]


def nfold_many(N, states, seeds, tables, seg_steps, clock, first_seg=0, need_in=None, events_in=None, traces=None):
    """nfold over the rows of `states`, stacked like the library's outputs.  `traces` (a list) receives the trace of every chain."""
    rows = [nfold(N, s, int(seeds[r]), tables, seg_steps, clock, first_seg, None if need_in is None else int(need_in[r]),
                  0 if events_in is None else int(events_in[r]), None if traces is None else _trace_of(traces))
            for r, s in enumerate(np.asarray(states).reshape(-1, N * N))]
    return {k: np.stack([np.asarray(r[k]) for r in rows]) for k in FIELDS + ("energy_hist",)}


def assert_equal(got, want, what, fields=FIELDS + ("energy_hist",)):
    for k in fields:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert [int(v) for v in a.reshape(-1)] == [int(v) for v in b.reshape(-1)] and a.shape == b.shape, f"{what}: {k}"
