"""Weight tables a CALLER may hand to the heat-bath entry points, which abi.heatbath_table never builds (its rows start at 2^24, fall
monotonically and are zero from the first zero on), and the two host entry points on a caller's table.  Every entry is at most
B = 2^24, the bound of include/mcq.h (item 3 of either heat-bath rule)."""
import numpy as np

import mcq_amd

abi = mcq_amd.abi
B = 1 << abi.HEATBATH_WEIGHT_BITS

ZERO_ROWS = ("zero", "zero3")  # W = 0 on every update
SPARSE = ("only1", "only3")    # T[0] = 0: W = 0 wherever no candidate lies at that distance from the minimum


def tables(n_sweeps):
    """{name: uint32[n_sweeps][D]}, what each family reaches:
    zero, zero3  D = 1 and D = 3, all 0: W = 0 on every update
    ones         D = 1, T = [1]: W = the number of candidates, the smallest non-zero W
    clip         [1, B]: the clip to D - 1 lands on a non-zero entry, so every far cell carries the large weight
    only1        [0, B, 0]: T[0] = 0 and weight on distance 1 only; W = 0 for some updates of a chain and not for others
    only3        [0, 0, 0, 7, 0]: the same, further out
    nonmono      [3, B, 0, 5, 1]: non-monotone with a zero in the middle
    rand         D = 6, RandomState(5).randint(0, B + 1), a different row per sweep: the per-sweep restaging
    altzero      rows [B, 1000, 1] / [0, 0, 0] / [5, 0, B] in turn: a zero row between two live ones
    full         D = 512, all B: the largest W and the largest partial sums the bound allows"""
    def rep(row):
        return np.tile(np.array([row], dtype=np.uint32), (n_sweeps, 1))

    alt = ([B, 1000, 1], [0, 0, 0], [5, 0, B])
    t = {"zero": rep([0]), "zero3": rep([0, 0, 0]), "ones": rep([1]), "clip": rep([1, B]), "only1": rep([0, B, 0]), "only3": rep([0, 0, 0, 7, 0]),
         "nonmono": rep([3, B, 0, 5, 1]), "rand": np.random.RandomState(5).randint(0, B + 1, size=(n_sweeps, 6)).astype(np.uint32),
         "altzero": np.array([alt[s % 3] for s in range(n_sweeps)], dtype=np.uint32).reshape(n_sweeps, 3), "full": rep([B] * abi.MAX_HEATBATH_TABLE)}
    assert all(v.dtype == np.uint32 and v.shape[0] == n_sweeps and int(v.max(initial=0)) <= B for v in t.values())
    return t


def host3d(N, Q, states, seeds, table, n_sweeps, first_sweep=0):
    """mcq_heatbath3d_host on a caller's table (heatbath_queens_host builds its own from betas)."""
    s = np.ascontiguousarray(states, dtype=np.uint8).reshape(len(seeds), 3 * Q)
    n = len(s)
    sd, tab = np.ascontiguousarray(seeds, dtype=np.uint32), np.ascontiguousarray(table, dtype=np.uint32)
    out = {"state": np.zeros_like(s), "best_state": np.zeros_like(s), "energy_hist": np.zeros((n, n_sweeps + 1), dtype=np.int32)}
    for k, dt in abi.HEATBATH3D_DTYPES.items():
        out[k] = np.zeros(n, dtype=dt)
    q = abi.Heatbath3D()
    q.N, q.n_queens, q.n_chains, q.n_sweeps, q.first_sweep, q.table_len = N, Q, n, n_sweeps, first_sweep, tab.shape[1]
    q.seeds, q.table, q.state_in, q.hist_stride = sd.ctypes.data, tab.ctypes.data, s.ctypes.data, n_sweeps + 1
    q.state_out = out["state"].ctypes.data
    for k in tuple(abi.HEATBATH3D_DTYPES) + ("best_state", "energy_hist"):
        setattr(q, k, out[k].ctypes.data)
    mcq_amd._lib.heatbath3d_host(q)
    return out


def host_with_table(N, s, seeds, tab, first_sweep, trace):
    """mcq_heatbath_host with the caller's own weight table uint32[n_sweeps][D]."""
    s, seeds, tab = np.ascontiguousarray(s, dtype=np.uint8), np.ascontiguousarray(seeds, dtype=np.uint32), np.ascontiguousarray(tab, dtype=np.uint32)
    n, n_sweeps = s.shape[0], tab.shape[0]
    out = {"state": np.zeros_like(s), "best_state": np.zeros_like(s)}
    for k, dt in abi.HEATBATH_DTYPES.items():
        out[k] = np.zeros(n, dtype=dt)
    q = abi.Heatbath()
    q.N, q.mode, q.n_chains, q.n_sweeps, q.first_sweep, q.table_len = N, abi.MODE_BOARD, n, n_sweeps, first_sweep, tab.shape[1]
    q.seeds, q.table = seeds.ctypes.data, tab.ctypes.data
    q.state_in, q.state_out, q.best_state = s.ctypes.data, out["state"].ctypes.data, out["best_state"].ctypes.data
    for k in abi.HEATBATH_DTYPES:
        setattr(q, k, out[k].ctypes.data)
    if trace:
        out["energy_hist"] = np.zeros((n, n_sweeps + 1), dtype=np.int32)
        q.energy_hist, q.hist_stride = out["energy_hist"].ctypes.data, n_sweeps + 1
    mcq_amd._lib.heatbath_host(q)
    return out
