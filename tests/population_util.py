"""Helpers of the population annealing tests: the resampling rule of include/mcq.h restated with NumPy and Python integers (no code
shared with the library), a run composed on the host from _lib.run_host_from segments and that restatement, and the vectors both the
host plan and the plan kernel are tried on, the fold rule of a segment's summary, and device arrays between guard bytes."""
import collections
import functools

import numpy as np

import mcq_amd
from mcq_amd.checkpoint import Checkpoint

abi = mcq_amd.abi


def table(dbeta):
    """T[d] = floor(2^24 exp(-dbeta d)), d = 0 .. D - 1; D = 1 + the first d with T = 0, at most 2^16."""
    out = []
    for d in range(1 << 16):
        t = int(np.floor(np.float64(2.0**24) * np.exp(np.float64(-dbeta) * np.float64(d))))
        out.append(t)
        if t == 0:
            break
    return np.array(out, dtype=np.uint32)


def plan(energies, R, tab, offsets):
    """(parent int32[n], stats int64[n / R][3]) by the rule, exact wherever the rule is defined (R W < 2^64): C_r R and m W + U in uint64,
    which they fit; W, U and x W through Python ints.  W = 0 (a table whose reachable entries are all zero): no C_r R exceeds a key, and
    by include/mcq.h every slot takes r = R - 1, one distinct parent."""
    e = np.asarray(energies, dtype=np.int64)
    tab = np.asarray(tab).astype(np.uint64)
    n, D = len(e), len(tab)
    assert n % R == 0 and len(offsets) == n // R
    parent = np.zeros(n, dtype=np.int32)
    stats = np.zeros((n // R, 3), dtype=np.int64)
    for g in range(n // R):
        E = e[g * R: (g + 1) * R]
        emin = int(E.min())
        w = tab[np.minimum(E - emin, D - 1)]
        C = np.cumsum(w, dtype=np.uint64)
        W = int(C[-1])  # (entries below 2^32 and R <= 2^19: below 2^51, nothing wraps)
        assert R * W < 2**64, "the rule is defined for R W < 2^64"
        U = (int(offsets[g]) * W) >> 32
        if W == 0:
            p = np.full(R, R - 1, dtype=np.int64)
        else:
            assert U < W and (R - 1) * W + U < R * W
            keys = np.arange(R, dtype=np.uint64) * np.uint64(W) + np.uint64(U)
            p = np.searchsorted(C * np.uint64(R), keys, side="right")  # the smallest r with C_r R > key
        assert p.max() < R
        parent[g * R: (g + 1) * R] = g * R + p
        stats[g] = (len(np.unique(p)), W, emin)
    return parent, stats


def plan_int64(energies, R, tab, offsets):
    """The restatement as it stood while every vector kept R W below 2^62: int64 throughout, W > 0 only.  Kept for one CPU test, which
    holds plan() to it on every vector of plan_vectors()."""
    e = np.asarray(energies, dtype=np.int64)
    tab = np.asarray(tab, dtype=np.int64)
    n, D = len(e), len(tab)
    assert n % R == 0 and len(offsets) == n // R
    parent = np.zeros(n, dtype=np.int32)
    stats = np.zeros((n // R, 3), dtype=np.int64)
    for g in range(n // R):
        E = e[g * R: (g + 1) * R]
        emin = int(E.min())
        w = tab[np.minimum(E - emin, D - 1)]
        C = np.cumsum(w)
        W = int(C[-1])
        U = (int(offsets[g]) * W) >> 32
        assert W > 0 and R * W < 2**62
        keys = np.arange(R, dtype=np.int64) * W + U
        p = np.searchsorted(C * R, keys, side="right")  # the smallest r with C_r R > key
        assert p.max() < R
        parent[g * R: (g + 1) * R] = g * R + p
        stats[g] = (len(np.unique(p)), W, emin)
    return parent, stats


def assert_plan_properties(energies, R, tab, parent, what):
    """Children counts are floor or ceil of R w / W, sum to R, and the map is monotone.  int64 arrays: R w < 2^51 for entries below 2^32 and
    R <= 2^19.  A population with W = 0 has no ratio to hold and is skipped."""
    e = np.asarray(energies, dtype=np.int64)
    tab = np.asarray(tab).astype(np.int64)
    D = len(tab)
    for g in range(len(e) // R):
        E = e[g * R: (g + 1) * R]
        w = tab[np.minimum(E - E.min(), D - 1)]
        W = int(w.sum())
        if W == 0:
            continue
        assert int(w.max()) * R < 2**51
        p = np.asarray(parent[g * R: (g + 1) * R], dtype=np.int64) - g * R
        assert p.min() >= 0 and p.max() < R, what
        assert (np.diff(p) >= 0).all(), f"{what}: parents are not monotone"
        kids = np.bincount(p, minlength=R)
        assert int(kids.sum()) == R, what
        lo, hi = (R * w) // W, -((-R * w) // W)
        bad = np.flatnonzero((kids < lo) | (kids > hi))
        assert len(bad) == 0, f"{what}: chain {int(bad[0])} of population {g} has {int(kids[bad[0]])} children, R w / W = {R * int(w[bad[0]])} / {W}"


def assert_plan_properties_walk(energies, R, tab, parent, what):
    """assert_plan_properties as a walk over Python ints, chain by chain (W > 0 only): what the vectorised form is held to, up to R = 1 024."""
    e = np.asarray(energies, dtype=np.int64)
    D = len(tab)
    for g in range(len(e) // R):
        E = e[g * R: (g + 1) * R]
        w = [int(tab[min(int(x) - int(E.min()), D - 1)]) for x in E]
        W = sum(w)
        p = np.asarray(parent[g * R: (g + 1) * R], dtype=np.int64) - g * R
        assert p.min() >= 0 and p.max() < R, what
        assert (np.diff(p) >= 0).all(), f"{what}: parents are not monotone"
        kids = np.bincount(p, minlength=R)
        assert int(kids.sum()) == R, what
        for r in range(R):
            lo, hi = (R * w[r]) // W, -((-R * w[r]) // W)
            assert lo <= int(kids[r]) <= hi, f"{what}: chain {r} of population {g} has {int(kids[r])} children, R w / W = {R * w[r]} / {W}"


def plan_vectors():
    """(name, energies, R, table, offsets): the adversarial vectors of the plan tests."""
    rs = np.random.RandomState(2024)
    X = (0, 1, 2**31, 2**32 - 1)
    t02, t0, t5 = table(0.02), table(0.0), table(5.0)
    assert len(t0) == 1 << 16 and t0[-1] == 1 << 24, "a table capped at 2^16"
    out = []
    for R in (16, 48, 1024, 65536):
        for x in X:
            out.append((f"equal energies R={R} x={x}", np.full(R, 77, dtype=np.int32), R, t02, [x]))
        far = np.full(R, 400, dtype=np.int32)
        far[R // 3] = 3
        out.append((f"one chain far below R={R}", far, R, t02, [X[R % 4]]))
        spread = rs.randint(0, 5000, size=R).astype(np.int32)  # beyond D - 1 = 832: the clamp
        out.append((f"spread beyond the table R={R}", spread, R, t02, [12345]))
        out.append((f"capped table R={R}", rs.randint(0, 200000, size=R).astype(np.int32), R, t0, [2**32 - 1]))
        out.append((f"sharp table R={R}", rs.randint(20, 30, size=R).astype(np.int32), R, t5, [2**31]))
        out.append((f"mild spread R={R}", rs.randint(100, 160, size=R).astype(np.int32), R, t02, [rs.randint(0, 2**32, dtype=np.uint32)]))
    for R, pops in ((16, 5), (48, 3), (1024, 4)):
        e = rs.randint(0, 300, size=R * pops).astype(np.int32)
        e[R: 2 * R] = 9
        out.append((f"{pops} populations of {R}", e, R, t02, [X[g % 4] for g in range(pops)]))
    bimodal = np.where(rs.rand(65536) < 0.1, 26, 140).astype(np.int32) + rs.randint(0, 6, size=65536).astype(np.int32)
    out.append(("bimodal R=65536", bimodal, 65536, t02, [987654321]))
    return out


Vector = collections.namedtuple("Vector", "group name energies R table offsets conds")
WIDE_SIZES = (80, 112, 1008, 1040, 2000, 65552, 1 << 19)
WIDE_GROUPS = tuple(f"R={R}" for R in WIDE_SIZES) + ("minimum", "range", "several", "entries")
INT_MIN, INT_MAX = -2**31, 2**31 - 1


def _weights(v):
    """w_r of every chain of a vector, from its inputs alone: int64[n / R][R]."""
    E = np.asarray(v.energies, dtype=np.int64).reshape(-1, v.R)
    return np.asarray(v.table).astype(np.int64)[np.minimum(E - E.min(axis=1, keepdims=True), len(v.table) - 1)]


def wide_vector_list():
    """The vectors the plan kernels were never launched on (plan_vectors() stays as it is): population sizes that leave the last
    wavefront or the last tile of 1 024 ragged, up to MCQ_MAX_POPULATION; caller's tables; the minimum in every corner of the workgroup; the
    whole int32 range; launches whose population boundaries fall inside wavefronts; entries beyond 2^24.  Every vector names, in `conds`,
    what it exists for; assert_conditions() holds it to that from the inputs and the restatement alone."""
    rs = np.random.RandomState(4242)
    word = lambda: int(rs.randint(0, 2**32, dtype=np.uint32))  # noqa: E731
    t02, t5 = table(0.02), table(0.5)
    heavy = ((1 << 24) - rs.randint(0, 1000, size=512)).astype(np.uint32)  # a caller's table: entries in (2^24 - 1000, 2^24], not monotone
    assert heavy.min() > (1 << 24) - 1000 and heavy.max() <= 1 << 24 and (np.diff(heavy.astype(np.int64)) > 0).any() and (np.diff(heavy.astype(np.int64)) < 0).any()
    t_zero0 = t02.copy()
    t_zero0[0] = 0
    capped = table(0.0).copy()  # D = 2^16 with entries D - 2 and D - 1 apart from the rest and from each other
    D = len(capped)
    capped[D - 2], capped[D - 1] = 3 << 22, 1 << 22
    out = []
    for R in WIDE_SIZES:
        grp, mild = f"R={R}", lambda: rs.randint(100, 160, size=R).astype(np.int32)  # noqa: E731
        out.append(Vector(grp, f"mild spread R={R}", mild(), R, t02, [word()], {"moves": True}))
        conds = {"moves": True}
        if R >= 1008:
            conds["W_at_least"] = 2**32
        if R == 1 << 19:
            conds["W_above"] = 2**42
        out.append(Vector(grp, f"heavy table R={R}", rs.randint(0, 600, size=R).astype(np.int32), R, heavy, [2**32 - 1], conds))
        out.append(Vector(grp, f"all-zero table R={R}", mild(), R, np.zeros(8, dtype=np.uint32), [word()], {"W_zero": True}))
        out.append(Vector(grp, f"T[0] = 0 R={R}", mild(), R, t_zero0, [word()], {"zero_weight_minimum": True, "moves": True}))
        out.append(Vector(grp, f"D = 1 R={R}", rs.randint(0, 5000, size=R).astype(np.int32), R, np.array([1 << 24], dtype=np.uint32), [word()], {"identity": True}))
        e = rs.randint(0, 70000, size=R).astype(np.int32)
        e[1], e[2], e[3], e[4], e[R - 1] = 0, D - 2, D - 1, D, 2 * D
        out.append(Vector(grp, f"D = 2^16 R={R}", e, R, capped, [word()], {"clamp_hits": D, "moves": True}))
    # a unique minimum in the corners of the scan kernel's workgroup: slot 0, slot R - 1, the first and the last slot of wavefront 15 and,
    # at R = 2 000, the ragged second tile (its wavefront 15 holds slots 1 984 .. 1 999)
    for R, slots in ((1024, (0, 960, 1023)), (2000, (0, 960, 1023, 1500, 1984, 1999))):
        for s in slots:
            e = (70 + rs.randint(0, 60, size=R)).astype(np.int32)
            e[s] = 50
            out.append(Vector("minimum", f"minimum in slot {s} R={R}", e, R, t5, [word()], {"minimum_at": s}))
    for R in (80, 1040):
        for how in ("first", "last", "negative"):
            e = rs.randint(INT_MIN + 1, INT_MAX, size=R).astype(np.int64)
            near = rs.permutation(R)[: R // 2]
            e[near] = INT_MIN + rs.randint(1, 700, size=len(near))
            if how == "negative":
                e = np.where(e >= 0, -1 - e, e)
                e[R // 2], e[5] = INT_MIN, -1
                conds = {"all_negative": True, "moves": True}
            else:
                lo, hi = (0, R - 1) if how == "first" else (R - 1, 0)
                e[lo], e[hi] = INT_MIN, INT_MAX
                conds = {"full_range": lo, "moves": True}
            out.append(Vector("range", f"int32 range, minimum {how} R={R}", e.astype(np.int32), R, t02, [word()], conds))
    for pops, R in ((13, 80), (5, 1040), (3, 2000), (9, 112)):
        e = rs.randint(0, 300, size=R * pops).astype(np.int32)
        e[R: 2 * R] = 9
        x = [0 if g == 0 else word() for g in range(pops)]
        out.append(Vector("several", f"{pops} populations of {R}", e, R, t02, x, {"inside_groups": True, "identity_populations": (1,), "x_zero": 0, "moves": True}))
    big = rs.randint(2**31, 2**32, size=64, dtype=np.uint64).astype(np.uint32)
    for R in (16, 80, 1024):
        out.append(Vector("entries", f"entries in [2^31, 2^32) R={R}", rs.randint(0, 100, size=R).astype(np.int32), R, big, [word()],
                          {"wave_prefix_above": 2**32, "moves": True}))
    for v in out:
        v.energies.setflags(write=False)
        assert v.group in WIDE_GROUPS and v.energies.dtype == np.int32
    for t in (t02, t5, heavy, t_zero0, capped, big):
        t.setflags(write=False)
    return out


def assert_conditions(v, parent, stats):
    """What the vector exists for, from its inputs and the restatement's (parent, stats) -- never from a kernel's output."""
    R, n = v.R, len(v.energies)
    E = np.asarray(v.energies, dtype=np.int64).reshape(-1, R)
    p = np.asarray(parent, dtype=np.int64).reshape(-1, R) - np.arange(n // R)[:, None] * R
    w, c, what = _weights(v), dict(v.conds), v.name
    same = set(c.pop("identity_populations", ()))
    for g in range(n // R):
        kids = np.bincount(p[g], minlength=R)
        if c.get("identity") or g in same:
            assert (p[g] == np.arange(R)).all() and int(stats[g, 0]) == R, f"{what}: population {g} is not the identity"
        elif c.get("moves"):
            assert (p[g] != np.arange(R)).any() and int(stats[g, 0]) < R, f"{what}: population {g} resamples nothing"
        if c.get("W_zero"):
            assert int(stats[g, 1]) == 0 and (p[g] == R - 1).all() and int(stats[g, 0]) == 1, what
        if "W_at_least" in c:
            assert int(stats[g, 1]) >= c["W_at_least"], what
        if "W_above" in c:
            assert int(stats[g, 1]) > c["W_above"] and R * int(stats[g, 1]) < 2**64, what
        if c.get("zero_weight_minimum"):
            at_min = E[g] == E[g].min()
            assert at_min.any() and (w[g][at_min] == 0).all() and (kids[at_min] == 0).all() and int(stats[g, 1]) > 0, what
        if "clamp_hits" in c:
            d = set((E[g] - E[g].min()).tolist())
            assert {c["clamp_hits"] - 2, c["clamp_hits"] - 1, c["clamp_hits"]} <= d and max(d) > c["clamp_hits"] == len(v.table), what
        if "minimum_at" in c:
            s = c["minimum_at"]
            assert int(np.argmin(E[g])) == s and int((E[g] == E[g].min()).sum()) == 1 and int(stats[g, 2]) == int(E[g, s]), what
            assert int(kids[s]) > R // 2, f"{what}: the minimum takes {int(kids[s])} of {R} slots"
        if "full_range" in c:
            assert E[g].min() == INT_MIN and E[g].max() == INT_MAX and int(np.argmin(E[g])) == c["full_range"] and int(stats[g, 2]) == INT_MIN, what
            assert int((E[g] == INT_MIN).sum()) == 1 and int(kids[c["full_range"]]) > 0
        if c.get("all_negative"):
            assert E[g].max() == -1 and E[g].min() == INT_MIN and int(stats[g, 2]) == INT_MIN, what
        if "wave_prefix_above" in c:
            assert R * int(stats[g, 1]) < 2**52, what
            assert any(int(np.cumsum(w[g][a: a + 64]).max()) > c["wave_prefix_above"] for a in range(0, R, 64)), what
            assert int(np.cumsum(w[g][:64])[min(R, 64) - 2]) > c["wave_prefix_above"], f"{what}: no prefix above 2^32 that a later lane of the wavefront adds to"
    if "x_zero" in c:
        assert int(v.offsets[c["x_zero"]]) == 0 and c["x_zero"] not in same, what
    if c.get("inside_groups"):
        cuts = np.arange(1, n // R) * R
        assert ((cuts % 64 != 0) & (cuts % 256 != 0)).any() and R > 64, f"{what}: no population boundary strictly inside a 64-slot and a 256-slot group"
        assert len(same) > 0


@functools.lru_cache(maxsize=None)
def wide_plans():
    """((vector, parent, stats), ...) of wide_vector_list() by the restatement: computed once, shared by the tests, read-only; every
    vector's condition is asserted here, before anything is compared with it."""
    out = []
    for v in wide_vector_list():
        p, s = plan(v.energies, v.R, v.table, v.offsets)
        p.setflags(write=False), s.setflags(write=False)
        assert_conditions(v, p, s)
        out.append((v, p, s))
    return tuple(out)


# ---- the fold of a segment's summary, and arrays between guard bytes (tests/test_near_ties.py, tests/test_population.py) -------------

GUARD = 0xA5
FOLD_SLOTS = 4096


def fold_rule(first_step, seg, run):
    """include/mcq.h, mcq_resample: a segment moves best_energy / steps_to_best (in whole-run steps) / best_state only by a STRICTLY lower
    energy; n_accepted, near_ties and stream_words (modulo 2^32) add up; first_step == 0 copies.  `seg`, `run`: dicts of arrays; returns
    the run's arrays after the fold."""
    first = first_step == 0
    lower = np.ones(len(seg["best_energy"]), dtype=bool) if first else seg["best_energy"] < run["best_energy"]
    out = {"best_energy": np.where(lower, seg["best_energy"], run["best_energy"]).astype(np.int32),
           "steps_to_best": np.where(lower, np.int64(first_step) + seg["steps_to_best"], run["steps_to_best"]).astype(np.int64),
           "n_accepted": (seg["n_accepted"] + (0 if first else run["n_accepted"])).astype(np.int64)}
    if "near_ties" in run:
        out["near_ties"] = (seg["near_ties"] + (0 if first else run["near_ties"])).astype(np.int64)
    if "stream_words" in run:
        out["stream_words"] = ((seg["stream_words"].astype(np.uint64) + (0 if first else run["stream_words"].astype(np.uint64))) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    if "best_state" in run:
        out["best_state"] = np.where(lower[:, None], seg["best_state"], run["best_state"])
    return out


def fold_vectors(first_step, state_bytes, seed, n=FOLD_SLOTS):
    """Random summaries of n slots with, in known numbers of slots: ties on both sides, stream words whose sum passes 2^32, steps
    beyond 2^31, equal best energies, and lower ones."""
    rs = np.random.RandomState(seed)
    seg = {"best_energy": rs.randint(0, 60, n).astype(np.int32), "steps_to_best": rs.randint(0, 5000, n).astype(np.int64),
           "n_accepted": rs.randint(0, 5000, n).astype(np.int64), "near_ties": np.zeros(n, dtype=np.int64),
           "stream_words": rs.randint(0, 2**31, n).astype(np.uint32), "best_state": rs.randint(0, 256, (n, state_bytes)).astype(np.uint8)}
    run = {"best_energy": rs.randint(0, 60, n).astype(np.int32), "steps_to_best": rs.randint(0, 2**40, n).astype(np.int64),
           "n_accepted": rs.randint(0, 2**40, n).astype(np.int64), "near_ties": np.zeros(n, dtype=np.int64),
           "stream_words": rs.randint(0, 2**31, n).astype(np.uint32), "best_state": rs.randint(0, 256, (n, state_bytes)).astype(np.uint8)}
    idx = rs.permutation(n)
    seg["near_ties"][idx[:700]] = rs.randint(1, 9, 700)                       # ties in the segment only, in the run only, on both sides
    run["near_ties"][idx[400:1100]] = rs.randint(1, 2**33, 700)
    wrap = idx[1100:1600]                                                     # 500 slots whose words pass 2^32
    seg["stream_words"][wrap] = rs.randint(2**31 + 1, 2**32, 500).astype(np.uint32)
    run["stream_words"][wrap] = rs.randint(2**31 + 1, 2**32, 500).astype(np.uint32)
    equal = idx[1600:2100]                                                    # 500 ties of the best energy: the run's values stay
    seg["best_energy"][equal] = run["best_energy"][equal]
    lower = idx[2100:2600]                                                    # 500 strictly lower: all three move
    seg["best_energy"][lower] = run["best_energy"][lower] - rs.randint(1, 5, 500).astype(np.int32)
    seg["steps_to_best"][idx[2600:3100]] = rs.randint(2**31, 2**33, 500)     # a segment's own step beyond 2^31
    counts = {"seg_ties": int((seg["near_ties"] > 0).sum()), "run_ties": int((run["near_ties"] > 0).sum()),
              "both_ties": int(((seg["near_ties"] > 0) & (run["near_ties"] > 0)).sum()),
              "wraps": int((seg["stream_words"].astype(np.uint64) + run["stream_words"].astype(np.uint64) >= 2**32).sum()),
              "equal": int((seg["best_energy"] == run["best_energy"]).sum()), "lower": int((seg["best_energy"] < run["best_energy"]).sum()),
              "far_steps": int((np.int64(first_step) + seg["steps_to_best"] > 2**31).sum())}
    return seg, run, counts


def guarded(torch, dev, a):
    """`a` on the device between two guard blocks of 64 bytes: (tensor of everything, view of the array)."""
    raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    buf = torch.full((raw.size + 128,), GUARD, dtype=torch.uint8, device=dev)
    buf[64: 64 + raw.size] = torch.from_numpy(raw.copy()).to(dev)
    return buf, buf[64: 64 + raw.size]


BOUNDARY_CHAINS, BOUNDARY_POPULATION = 4160, 1040


def boundary_vectors(first_step, state_bytes, seed):
    """What anneal_population hands mcq_resample_device at an inner boundary, 4 populations of 1 040 slots: the finished segment's energies,
    placements and summary, the run's summary so far, a table and the offset words.  Returns the inputs, the restatement's plan and the
    counts the tests require of them."""
    n, R = BOUNDARY_CHAINS, BOUNDARY_POPULATION
    seg, run, counts = fold_vectors(first_step, state_bytes, seed, n=n)
    rs = np.random.RandomState(seed + 1000)
    v = {"energies": rs.randint(20, 120, size=n).astype(np.int32), "state": rs.randint(0, 256, size=(n, state_bytes)).astype(np.uint8),
         "offsets": rs.randint(0, 2**32, size=n // R, dtype=np.uint32), "table": table(0.05), "seg": seg, "run": run, "R": R}
    v["parent"], v["stats"] = plan(v["energies"], R, v["table"], v["offsets"])
    counts["moved"] = int((v["parent"] != np.arange(n)).sum())
    v["counts"] = counts
    return v


def merge_rule(ckpt, seg, seg_steps, received=None):
    """Checkpoint.merge for a slot that took over a parent's placement: the checkpoint first stands at the energy the slot RECEIVED (merge
    then checks that the segment's recounted initial energy is exactly that)."""
    if received is not None:
        ckpt.energy = np.asarray(received).astype(np.int64)
    return ckpt.merge(seg, seg_steps)


def compose_host(N, n_steps, init_mode, sp, seeds, S, population=None, resample_seed=0, mcmc_type="board", trace=False, lanes_per_chain=0, Q=None):
    """The run anneal_population makes, composed on the host: _lib.run_host_from segments, plan() in between, Checkpoint.merge per slot.
    Returns (res, lineage) with the fields of anneal_population."""
    seeds = np.asarray(seeds, dtype=np.uint32)
    n = len(seeds)
    R = n if population is None else population
    K = -(-n_steps // S)
    lengths = [S] * (K - 1) + [n_steps - (K - 1) * S]
    beta = abi.beta_values(sp, n_steps)
    offsets = np.random.RandomState(resample_seed).randint(0, 2**32, size=(K - 1, n // R), dtype=np.uint32)
    ckpt = Checkpoint(N, mcmc_type, n_steps, seeds, schedule_params=sp, Q=Q, trace=trace)
    segs, parents, stats, received = [], [], [], []
    state = stream_state = recv = None
    near = np.zeros(n, dtype=np.int64)
    for k, L in enumerate(lengths):
        p = abi.make_params(N, L, init_mode, sp, n, mcmc_type=mcmc_type, trace=trace, lanes_per_chain=lanes_per_chain, Q=Q)
        r = abi.make_resume(p, ckpt.step, n_steps, state=state, stream_state=stream_state)
        seg, _ = mcq_amd._lib.run_host_from(p, seeds, r, checkpoint=True, trace=trace, states=True)
        merge_rule(ckpt, seg, L, recv)
        near += seg["near_ties"]
        segs.append(seg)
        stream_state = seg["stream_state"]
        if k < K - 1:
            par, st = plan(seg["final_energy"], R, table(beta[(k + 1) * S] - beta[k * S]), offsets[k])
            state, recv = seg["final_state"][par], seg["final_energy"][par]
            parents.append(par), stats.append(st), received.append(recv)
    res = {
        "hist_len": np.full(n, n_steps + 1, dtype=np.int64), "steps_executed": np.full(n, n_steps, dtype=np.int64),
        "initial_energy": segs[0]["initial_energy"], "final_energy": segs[-1]["final_energy"], "best_energy": ckpt.best_energy.astype(np.int32),
        "steps_to_best": ckpt.steps_to_best.astype(np.int64), "n_accepted": ckpt.n_accepted.astype(np.int64), "near_ties": near,
        "stream_words": (ckpt.stream_words & np.uint64(0xFFFFFFFF)).astype(np.uint32), "stream_state": stream_state,
        "best_state": ckpt.best_state, "final_state": segs[-1]["final_state"],
    }
    if trace is True:
        hist = np.zeros((n, abi.hist_stride_for(n_steps)), dtype=np.int32)
        bits = np.zeros((n, abi.bits_stride_for(n_steps) * 64), dtype=np.uint8)
        done = 0
        for s, L in zip(segs, lengths):
            if done == 0:
                hist[:, : L + 1] = s["energy_hist"][:, : L + 1]
            else:
                hist[:, done + 1: done + L + 1] = s["energy_hist"][:, 1: L + 1]
            bits[:, done: done + L] = np.unpackbits(np.ascontiguousarray(s["accept_bits"]).view(np.uint8), axis=1, bitorder="little")[:, :L]
            done += L
        res["energy_hist"] = hist
        res["accept_bits"] = np.ascontiguousarray(np.packbits(bits, axis=1, bitorder="little")).view(np.uint64)
    elif trace == "reduced":
        for key in ("step_sum", "step_sumsq", "step_accepted", "step_count"):
            res[key] = np.concatenate([s[key] if i == 0 else s[key][1:] for i, s in enumerate(segs)])
    par = np.array(parents, dtype=np.int32).reshape(K - 1, n)
    sts = np.array(stats, dtype=np.int64).reshape(K - 1, n // R, 3)
    anc = np.arange(n, dtype=np.int32)
    for q in par:
        anc = anc[q]
    lineage = {"parents": par, "distinct_parents": sts[:, :, 0], "weight_sum": sts[:, :, 1], "e_min": sts[:, :, 2], "ancestors": anc,
               "segment_initial_energy": np.array([s["initial_energy"] for s in segs]), "segment_final_energy": np.array([s["final_energy"] for s in segs]),
               "received_energy": np.array(received, dtype=np.int32).reshape(K - 1, n)}
    return res, lineage


LINEAGE_FIELDS = ("parents", "distinct_parents", "weight_sum", "e_min", "ancestors", "segment_initial_energy", "segment_final_energy", "received_energy")
RESULT_FIELDS = ("hist_len", "steps_executed", "initial_energy", "final_energy", "best_energy", "steps_to_best", "n_accepted", "near_ties",
                 "stream_words", "stream_state", "best_state", "final_state")
TRACE_FIELDS = {True: ("energy_hist", "accept_bits"), "reduced": ("step_sum", "step_sumsq", "step_accepted", "step_count"), False: ()}


def assert_runs_equal(got, want, trace, what):
    (res, lin), (hres, hlin) = got, want
    for k in RESULT_FIELDS + TRACE_FIELDS[trace]:
        assert k in res and k in hres, f"{what}: {k} missing"
        np.testing.assert_array_equal(res[k], hres[k], err_msg=f"{what}: {k}")
    for k in LINEAGE_FIELDS:
        np.testing.assert_array_equal(lin[k], hlin[k], err_msg=f"{what}: lineage {k}")
