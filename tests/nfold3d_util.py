"""The n-fold rule of full_3d placements (include/mcq.h: mcq_nfold3d) restated in NumPy and Python integers, from the text of the rule
and from nothing else: what mcq_nfold3d_host and the kernel are compared with.  A brute force over all (q, t) pairs behind every
event; Philox is this file's own, tau, the 96-bit product and U are Python integers, and the attack is that of tests/quench3d_util.py."""
import functools

import numpy as np

from tests import quench3d_util as q3

MASK = 0xFFFFFFFF
KEY_WORD = 12
TIME_BITS = 12
FIELDS = ("state", "best_state", "energy_in", "energy_out", "best_energy", "best_step", "events_out", "n_uphill", "n_flat", "need_out", "weight_out",
          "flags")


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
    """Block e of the chain seeded `seed` (rule item 4)."""
    return philox((e & MASK, e >> 32, 0, 0), (int(seed), KEY_WORD))


def ell(x, ln2, clock_table):
    """l(x) = z clock_ln2 + clock_table[y]: z leading zero bits, y the 8 bits below the leading one bit (zeros where there are none)."""
    x = int(x)
    if x == 0:
        return 32 * int(ln2) + int(clock_table[0])
    z = 32 - x.bit_length()
    y = (((x << z) & MASK) >> 23) & 255
    return z * int(ln2) + int(clock_table[y])


def index_of(N, z):
    return (z[:, 0] * N + z[:, 1]) * N + z[:, 2]


def weights(N, z, row):
    """(w, d) as int64 arrays [Q][N^3] of the clamped placement z (distinct cells) under the weight row `row`: d = a(q, t) - c_q with
    a(q, t) = S(t) - [pos(q) attacks t], w = row[clip(d, 0, D - 1)], and 0 in the columns of the cells that hold a queen."""
    att = q3.attack_matrix(q3._cells(N), z)  # bool[N^3][Q]
    S = att.sum(axis=1).astype(np.int64)
    idx = index_of(N, z)
    c = S[idx] - 1
    d = S[None, :] - att.T.astype(np.int64) - c[:, None]
    w = np.asarray(row, dtype=np.int64)[np.clip(d, 0, len(row) - 1)]
    w[:, idx] = 0
    return w, d


def nfold(N, placement, seed, tables, seg_steps, clock, first_seg=0, need_in=None, events_in=0, trace=None):
    """One placement through the rule; returns a dict with the fields of mcq_nfold3d plus `energy_hist`.  `trace` (a list) receives
    (segment, left, q, t, d, tau, U, W, lo, hi, zero_before) of every event: the chosen move holds the integers lo <= U < hi of
    0 .. W - 1, and zero_before says whether the move before it in walk order (q ascending, free cells ascending) has weight 0."""
    ln2, ct = clock
    z = q3.clamp(N, placement).copy()
    Q, C = len(z), N ** 3
    M = Q * (C - Q)
    E = q3.energy(N, z)
    e = int(events_in)
    x = block(seed, e)
    need = int(need_in) if need_in is not None else M * ell(x[2], ln2, ct)
    tables = np.asarray(tables)
    if q3.is_repeated(N, z):
        return {"state": z.astype(np.uint8).reshape(-1), "best_state": z.astype(np.uint8).reshape(-1), "energy_in": E, "energy_out": E, "best_energy": E,
                "best_step": 0, "events_out": e, "n_uphill": 0, "n_flat": 0, "need_out": need, "weight_out": 0, "flags": 1,
                "energy_hist": np.full(len(tables) + 1, E, dtype=np.int64)}
    e_in, best_e, best_step, best = E, E, 0, z.copy()
    up = flat = 0
    W = 0
    hist = [E]
    for s, row in enumerate(tables):
        whole = int(seg_steps) << TIME_BITS
        left = whole
        while True:
            w, d = weights(N, z, row)
            R = [int(v) for v in w.sum(axis=1)]
            W = sum(R)
            assert W <= M << 24
            if W == 0:
                break
            tau = max(1, (need << TIME_BITS) // W)
            if tau > left:
                spent = (left * W) >> TIME_BITS
                assert spent <= need
                need -= spent
                break
            left -= tau
            U = (((x[0] << 32) | x[1]) * W) >> 64
            sums = np.cumsum(w.reshape(-1))
            flat_index = int(np.searchsorted(sums, U, side="right"))  # the first inclusive prefix sum above U
            q, t = divmod(flat_index, C)
            assert w[q, t] > 0
            dd = int(d[q, t])
            if trace is not None:
                held = set(int(v) for v in index_of(N, z))
                before = flat_index - 1
                while before >= 0 and before % C in held:
                    before -= 1
                trace_tail = (int(sums[flat_index]) - int(w[q, t]), int(sums[flat_index]), bool(before >= 0 and w.reshape(-1)[before] == 0))
            z[q] = (t // (N * N), (t // N) % N, t % N)
            E += dd
            up += dd > 0
            flat += dd == 0
            e += 1
            if trace is not None:
                trace.append((s, left, q, t, dd, tau, U, W) + trace_tail)
            if E < best_e:
                best_e, best_step, best = E, s * int(seg_steps) + ((whole - left) >> TIME_BITS), z.copy()
            x = block(seed, e)
            need = M * ell(x[2], ln2, ct)
        hist.append(E)
    assert E == q3.energy(N, z) and not q3.is_repeated(N, z)
    return {"state": z.astype(np.uint8).reshape(-1), "best_state": best.astype(np.uint8).reshape(-1), "energy_in": e_in, "energy_out": E,
            "best_energy": best_e, "best_step": best_step, "events_out": e, "n_uphill": up, "n_flat": flat, "need_out": need,
            "weight_out": W if len(tables) else 0, "flags": 0, "energy_hist": np.array(hist, dtype=np.int64)}


def _trace_of(traces):
    traces.append([])
    return traces[-1]


def nfold_many(N, states, seeds, tables, seg_steps, clock, Q=None, first_seg=0, need_in=None, events_in=None, traces=None):
    """nfold over the rows of `states`, stacked like the library's outputs.  `traces` (a list) receives the trace of every chain."""
    Q = N * N if Q is None else Q
    rows = [nfold(N, s, int(seeds[r]), tables, seg_steps, clock, first_seg, None if need_in is None else int(need_in[r]),
                  0 if events_in is None else int(events_in[r]), None if traces is None else _trace_of(traces))
            for r, s in enumerate(np.asarray(states).reshape(-1, 3 * Q))]
    return {k: np.stack([np.asarray(r[k]) for r in rows]) for k in FIELDS + ("energy_hist",)}


def assert_equal(got, want, what, fields=FIELDS + ("energy_hist",)):
    for k in fields:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert [int(v) for v in a.reshape(-1)] == [int(v) for v in b.reshape(-1)], f"{what}: {k}"


def moves(N, before, after):
    """(queens, cells): the queens whose cell differs between two stacks of placements uint8[n][3 Q], and the cell index each ended on."""
    b = np.minimum(np.asarray(before, dtype=np.int64).reshape(len(before), -1, 3), N - 1)
    a = np.asarray(after, dtype=np.int64).reshape(b.shape)
    r, q = np.nonzero((a != b).any(axis=2))
    return q, (a[r, q, 0] * N + a[r, q, 1]) * N + a[r, q, 2]


def shares(N, Q):
    """The runs the kernel gives its first and its last busy lane: ((queens of lane 0), (queens of the last lane), (cells of lane 0),
    (cells of the last lane)), each as a half-open range -- a contiguous run of ceil(Q / W) queens per lane, and of ceil(dwords / W) | 1
    field dwords, W = 64, 256 or 1024 lanes and 4 or 2 cells per dword as csrc/mcq_field.h lays them out."""
    W, cpd = (64, 4) if N <= 12 else (256, 4) if N <= 19 else (1024, 2)
    C = N ** 3
    qc = -(-Q // W)
    fw = -(-C // cpd)
    rw = -(-fw // W) | 1
    last_q = (Q - 1) // qc * qc
    last_w = (fw - 1) // rw * rw
    return (0, min(qc, Q)), (last_q, Q), (0, min(rw * cpd, C)), (last_w * cpd, C)


def q3_placement(N, cells):
    """uint8[3 Q]: the placement whose queens hold the cells `cells` (indices), in that order."""
    c = np.asarray(cells, dtype=np.int64)
    return np.stack([c // (N * N), (c // N) % N, c % N], axis=1).astype(np.uint8).reshape(-1)


def largest_queens(abi, N):
    """The largest Q whose chain fits the LDS of a workgroup at N."""
    return next(Q for Q in range(N ** 3 - 1, 1, -1) if abi.nfold3d_lds_bytes(N, Q) <= abi.MAX_NFOLD3D_LDS)


@functools.lru_cache(maxsize=None)
def wide_need_case(nfold, abi):
    """(placements, seeds, need_in, rows, the host code's result) of four chains at N = 32, Q = 1 024 under the row [1, 0], one segment of
    2^31 steps, the mean clock.  W, the number of moves that do not raise E, is about 2^24.  Chains 0 - 2 carry needs of 2^58 - 1,
    2^57 + 12345 and 3 2^55 + 1: need 2^12 >= 2^64, q1 = need div W >= 2^32, nothing fires and need -= floor(2^43 W / 2^12), a 96-bit
    product.  Chain 3 carries floor((2^43 - 5) W / 2^12) + 1, about 2^55: q1 < 2^32, tau = 2^43 - 5 from both quotients, the event
    fires with 5 units left, and the next need, M 2^24, does not fire within them."""
    from tests import quench3d_util as q3

    N, n = 32, 4
    s = q3.random_placements(N, n, 32)
    seeds = abi.seeds_for(4294967000, n)
    rows = np.array([[1, 0]], dtype=np.uint32)
    W = nfold.nfold_queens_host(N, s[3:], seeds[3:], rows, 1, clock="mean", need_in=np.array([1 << 57], dtype=np.uint64))["weight_out"]
    left = 1 << 43
    need = np.array([2**58 - 1, 2**57 + 12345, 3 * 2**55 + 1, (((left - 5) * int(W[0])) >> 12) + 1], dtype=np.uint64)
    want = nfold.nfold_queens_host(N, s, seeds, rows, 1 << 31, clock="mean", need_in=need, hist=True)
    return s, seeds, need, rows, want


@functools.lru_cache(maxsize=None)
def aimed_case(N, Q):
    """(placements uint8[2][3 Q], seeds uint32[2]) whose FIRST event under a row of equal weights draws a cell of the first lane's run
    (chain 0) and of the last busy lane's run (chain 1).  With every weight 2^24, W = M 2^24 and the drawn pair is number
    floor(U / 2^24) in the order q ascending, free cells ascending, U = floor(X W / 2^64) from block 0 of the chain: the seeds are the
    first from 1 on whose pair has such a cell, found with this file's Philox."""
    s = q3.random_placements(N, 2, 900 + N, Q=Q)
    C = N ** 3
    F, M = C - Q, Q * (C - Q)
    runs = shares(N, Q)[2:]
    seeds = []
    for r, (lo, hi) in enumerate(runs):
        free = np.setdiff1d(np.arange(C), index_of(N, q3.clamp(N, s[r])))
        assert ((free >= lo) & (free < hi)).any()
        seed = 1
        while True:
            x = block(seed, 0)
            pair = ((((x[0] << 32) | x[1]) * (M << 24)) >> 64) >> 24
            if lo <= int(free[pair % F]) < hi:
                break
            seed += 1
        seeds.append(seed)
    return s, np.array(seeds, dtype=np.uint32)
