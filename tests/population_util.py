"""Helpers of the population annealing tests: the resampling rule of include/mcq.h restated with NumPy and Python integers (no code
shared with the library), a run composed on the host from _lib.run_host_from segments and that restatement, and the vectors both the
host plan and the plan kernel are tried on."""
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
    """(parent int32[n], stats int64[n / R][3]) by the rule: exact integers throughout (R W < 2^62 fits int64; x W goes through Python ints)."""
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
    """Children counts are floor or ceil of R w / W (Python ints), sum to R, and the map is monotone."""
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
