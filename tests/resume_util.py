"""Helpers of the checkpoint / resume tests: chains run in segments and stitched into the shape of one call's result, NumPy's own
stream walked to a word count, a pair-by-pair energy recount."""
import numpy as np

import mcq_amd

abi = mcq_amd.abi
ex = mcq_amd.experiments


def stitch(segments, lengths, ckpt, trace=True):
    """Segment results (experiments.start_chains / continue_chains, in order) -> one dict shaped like _lib.run_host's for the whole run:
    histories joined by dropping each later segment's entry 0, accept bits joined bit by bit, the summary from the merged checkpoint."""
    n, total = len(ckpt.seeds), int(sum(lengths))
    out = {
        "hist_len": np.full(n, total + 1, dtype=np.int64),
        "steps_executed": np.full(n, total, dtype=np.int64),
        "initial_energy": segments[0]["initial_energy"].copy(),
        "final_energy": segments[-1]["final_energy"].copy(),
        "best_energy": ckpt.best_energy.astype(np.int32),
        "steps_to_best": ckpt.steps_to_best.astype(np.int64),
        "n_accepted": ckpt.n_accepted.astype(np.int64),
        "best_state": ckpt.best_state,
        "final_state": ckpt.state,
        "stream_words": (ckpt.stream_words & np.uint64(0xFFFFFFFF)).astype(np.uint32),
        "near_ties": sum(s["near_ties"] for s in segments),
    }
    if trace is True:
        hist = np.zeros((n, abi.hist_stride_for(total)), dtype=np.int32)
        bits = np.zeros((n, total), dtype=np.uint8)
        done = 0
        for s, k in zip(segments, lengths):
            if done == 0:
                hist[:, : k + 1] = s["energy_hist"][:, : k + 1]
            else:
                np.testing.assert_array_equal(s["energy_hist"][:, 0], hist[:, done], err_msg="entry 0 of a segment repeats the last entry of the one before")
                hist[:, done + 1: done + k + 1] = s["energy_hist"][:, 1: k + 1]
            bits[:, done: done + k] = np.unpackbits(np.ascontiguousarray(s["accept_bits"]).view(np.uint8), axis=1, bitorder="little")[:, :k]
            done += k
        words = abi.bits_stride_for(total)
        padded = np.zeros((n, words * 64), dtype=np.uint8)
        padded[:, :total] = bits
        out["energy_hist"] = hist
        out["accept_bits"] = np.ascontiguousarray(np.packbits(padded, axis=1, bitorder="little")).view(np.uint64)
    elif trace == "reduced":
        for key in ("step_sum", "step_sumsq", "step_accepted", "step_count"):
            parts = [s[key] if i == 0 else s[key][..., 1:] for i, s in enumerate(segments)]  # entry 0 of a later segment is the entry before, again
            out[key] = np.concatenate(parts, axis=-1)
    return out


def run_in_segments(lengths, first, trace=True, **cont):
    """first: callable(n_steps) -> (res, ckpt) that runs the first segment; the rest through continue_chains.  Returns (segments, ckpt)."""
    res, ckpt = first(lengths[0])
    segs = [res]
    for k in lengths[1:]:
        res, ckpt = ex.continue_chains(ckpt, k, trace=trace, **cont)
        segs.append(res)
    return segs, ckpt


def cuts_to_lengths(cuts, total):
    edges = [0] + sorted(set(int(c) for c in cuts if 0 < c < total)) + [total]
    return [b - a for a, b in zip(edges[:-1], edges[1:])]


def numpy_state_after(start, n_words):
    """(key[624], position) NumPy itself holds after `n_words` more 32-bit words: `start` is a seed (int) or a uint32[625] state."""
    rs = np.random.RandomState()
    if np.ndim(start) == 0:
        rs.seed(int(start))
    else:
        rs.set_state(("MT19937", np.asarray(start[:624], dtype=np.uint32), int(start[624])))
    left = int(n_words)
    while left > 0:
        step = min(left, 1 << 22)
        rs.randint(0, 2**32, size=step, dtype=np.uint32)
        left -= step
    st = rs.get_state()
    return np.asarray(st[1], dtype=np.uint32), int(st[2])


def assert_stream_is_numpys(stream_state_row, start, n_words, what):
    key, pos = numpy_state_after(start, n_words)
    assert int(stream_state_row[624]) == pos, f"{what}: position {int(stream_state_row[624])}, NumPy stands at {pos} after {n_words} words"
    np.testing.assert_array_equal(stream_state_row[:624], key, err_msg=f"{what}: key after {n_words} words (position {pos})")


def recount(mode, N, row):
    """Attacking pairs of one state, pair by pair on the host: cells share a line iff all non-zero coordinate offsets have one magnitude."""
    if mode == "board":
        h = np.asarray(row, dtype=np.int64).reshape(N, N)
        i, j = np.meshgrid(np.arange(N), np.arange(N), indexing="ij")
        q = np.stack([i.ravel(), j.ravel(), h.ravel()], axis=1)
    else:
        q = np.asarray(row, dtype=np.int64).reshape(-1, 3)
    q = q.astype(np.int16)
    total = 0
    for a in range(0, len(q), 256):  # in slabs of rows: a board of N = 128 has 16 384 queens
        d = np.abs(q[a: a + 256, None, :] - q[None, :, :])
        mx = d.max(axis=2)
        ok = ((d == 0) | (d == mx[:, :, None])).all(axis=2) & (mx > 0)
        total += int(ok.sum())
    return total // 2  # every pair was seen from both ends
