"""CPU-only: which instantiation of mcq_sweep_kernel a launch takes (mcq_sweep_variant) against a recorded table.

Every variant computes the same results, so a wrong selection passes every parity test and only costs speed.  The table in
tests/golden/sweep_variants.npz was therefore recorded from the dispatch tree that preceded select_sweep_variant (DESIGN.md
section 4.2 has the recipe), over the grid below, for a device of 1 024 SIMDs -- the MI355X's count, and what the library
assumes when no device answers.  `python -m tests.test_sweep_variant LIB.so FUNCTION OUT.npz` records such a table from any
library that exports FUNCTION with mcq_sweep_variant's signature."""
import ctypes
import os
import re
import sys

import numpy as np

import mcq_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sweep_variants.npz")

N_STEPS = 1000
# 1 024 SIMDs: a board launch widens while n * 2G / 64 <= 1 024, the 8-lane kernels are "roomy" up to 16 384 chains, the 16-lane ones up to 8 192.
# 1 024 chains lie below all of these, 12 288 between the two roomy thresholds (and beyond any widening), 65 536 above all.
CHAINS = (1024, 12288, 65536)
LADDER = [1.0, 0.8, 0.6, 0.4]

# Instantiations the library holds that no parameter block reaches (the recording shows none of them): the dispatch tree that
# preceded the table named them behind a test that an earlier one had already taken -- boards up to N = 4 at 4 lanes always take
# the five-candidate kernels, so the plain one-pass kernels without a reduced trace never ran.  They stay built so that the code
# object stays what it was.
KNOWN_UNREACHED = {
    (0, 4, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0),
    (0, 4, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0),
}


def grid():
    """The parameter blocks of the recording, in its fixed order: every block is one validate() accepts, or refuses for its lane count."""
    abi = mcq_amd.abi
    sp = {"type": "constant", "beta_const": 1.0}
    for mode in ("board", "full_3d"):
        top = abi.MAX_N_BOARD if mode == "board" else abi.MAX_N
        for lanes in (0, 2, 4, 8, 16):
            for N in range(abi.MIN_N, top + 1):
                # full_3d: Q = N^2 and the largest other count the library takes; board: early stop off and within n_steps
                for second in (False, True):
                    Q = min(N**3 - 1, 32767) if mode == "full_3d" and second else None
                    patience = N_STEPS // 2 if mode == "board" and second else None
                    for trace in (False, True, "reduced"):
                        for rng in ("mt19937", "philox"):
                            for exchange in (False, True):
                                # what validate() refuses for other reasons than the lane count is not part of the grid
                                if exchange and (trace == "reduced" or patience is not None):
                                    continue
                                if mode == "full_3d" and N > 32 and (exchange or rng == "philox"):
                                    continue
                                for flags in (0, abi.FLAG_LINE_COUNTERS):
                                    for chains in CHAINS:
                                        p = abi.make_params(N, N_STEPS, "random", sp, chains, mcmc_type=mode, early_stop_patience=patience, trace=trace, flags=flags,
                                                            lanes_per_chain=lanes, rng=rng, Q=Q)
                                        if exchange:
                                            abi.set_exchange(p, 10, LADDER)
                                        yield p


def outcomes(fn, last_error):
    """fn over the grid: per point the 13 values of the variant and the LDS bytes per workgroup, or the return code and the message."""
    v, lds = (ctypes.c_int32 * 13)(), ctypes.c_int64()
    for p in grid():
        rc = fn(ctypes.byref(p), v, ctypes.byref(lds))
        yield (tuple(v), int(lds.value)) if rc == 0 else (int(rc), last_error().decode())


def pack(results):
    """Distinct variants and distinct refusals as lists, and per grid point an index (refusal k as -1 - k) and the LDS bytes."""
    variants, refusals, choice, lds = [], [], [], []
    for a, b in results:
        if isinstance(a, tuple):
            if a not in variants:
                variants.append(a)
            choice.append(variants.index(a)), lds.append(b)
        else:
            if (a, b) not in refusals:
                refusals.append((a, b))
            choice.append(-1 - refusals.index((a, b))), lds.append(0)
    return {"variants": np.array(variants, dtype=np.int32), "refusal_codes": np.array([c for c, _ in refusals], dtype=np.int32),
            "refusal_texts": np.array([t for _, t in refusals]), "choice": np.array(choice, dtype=np.int16), "lds_bytes": np.array(lds, dtype=np.int32)}


def _table_rows():
    """The rows of SWEEP_TABLE in csrc/mcq_hip.hip as tuples of 13 integers."""
    src = open(os.path.join(ROOT, "monte-carlo-collective_amd", "csrc", "mcq_hip.hip")).read()
    word = {"MCQ_MODE_BOARD": 0, "MCQ_MODE_FULL3D": 1, "false": 0, "true": 1}
    rows = [tuple(word[x] if x in word else int(x) for x in re.split(r",\s*", m)) for m in re.findall(r"^\s*SWEEP_ROW\(([^)]*)\),", src, flags=re.M)]
    assert all(len(r) == 13 for r in rows)
    return rows


def test_selection_matches_the_recorded_table():
    L = mcq_amd._lib.lib()
    assert L.mcq_device_simds() == 1024  # the recording's device; the selection looks at nothing else of it
    want = np.load(GOLDEN)
    got = pack(outcomes(L.mcq_sweep_variant, L.mcq_last_error))
    assert len(got["choice"]) == len(want["choice"]) == 85320
    # compared through the lists, so that the order in which variants first appear does not matter
    wv, gv = [tuple(r) for r in want["variants"]], [tuple(r) for r in got["variants"]]
    wr, gr = list(zip(want["refusal_codes"], want["refusal_texts"])), list(zip(got["refusal_codes"], got["refusal_texts"]))
    look = lambda c, vs, rs: vs[c] if c >= 0 else rs[-1 - c]  # noqa: E731
    bad = [i for i, (a, b) in enumerate(zip(want["choice"], got["choice"])) if look(a, wv, wr) != look(b, gv, gr)]
    assert not bad, (len(bad), bad[:10])
    assert (want["lds_bytes"] == got["lds_bytes"]).all()
    assert {t.split(" (")[0] for _, t in wr} == {"lanes_per_chain 2 applies to mcmc_type board", "full_3d beyond N = 32 runs at 16 lanes per chain", "chain state does not fit in LDS"}
    assert {int(c) for c, _ in wr} == {mcq_amd.abi.EINVAL}


def test_every_table_row_is_reached():
    """The 133 rows of the instantiation table against the recorded variants: every row is taken by some grid point but the known few."""
    rows = _table_rows()
    assert len(rows) == 133 and len(set(rows)) == 133
    recorded = {tuple(int(x) for x in r) for r in np.load(GOLDEN)["variants"]}
    assert recorded <= set(rows)
    assert set(rows) - recorded == KNOWN_UNREACHED


def test_jobs_lds_estimate_is_the_board_layout():
    """jobs._lds_bytes_per_wave restates the plain board layout in Python: equal to what a launch asks for, for every board and lane count."""
    abi, L = mcq_amd.abi, mcq_amd._lib.lib()
    v, lds = (ctypes.c_int32 * 13)(), ctypes.c_int64()
    n = 0
    for N in range(abi.MIN_N, abi.MAX_N_BOARD + 1):
        for lanes in (2, 4, 8, 16):
            p = abi.make_params(N, N_STEPS, "random", {"type": "constant", "beta_const": 1.0}, 1024, mcmc_type="board", lanes_per_chain=lanes)
            if L.mcq_sweep_variant(ctypes.byref(p), v, ctypes.byref(lds)) != 0:
                assert b"does not fit in LDS" in L.mcq_last_error() and mcq_amd.jobs._lds_bytes_per_wave(N, lanes) > 160 * 1024
                continue
            assert mcq_amd.jobs._lds_bytes_per_wave(N, lanes) == lds.value, (N, lanes)
            n += 1
    assert n > 400


def test_sweep_variant_wrapper_names_the_fields():
    p = mcq_amd.abi.make_params(24, N_STEPS, "random", {"type": "constant", "beta_const": 1.0}, 1024, mcmc_type="board", trace="reduced", lanes_per_chain=8)
    v = mcq_amd._lib.sweep_variant(p)
    assert tuple(v) == mcq_amd.abi.SWEEP_VARIANT_FIELDS + ("lds_bytes",) and v["lds_bytes"] == mcq_amd.jobs._lds_bytes_per_wave(24, 8)
    assert {k: x for k, x in v.items() if x and k != "lds_bytes"} == {"G": 8, "NT": 3, "REDUCED": 1, "NC": 24, "EARLYU": 1}
    p.N = 200
    try:
        mcq_amd._lib.sweep_variant(p)
        raise AssertionError("accepted N = 200")
    except ValueError as e:
        assert "N out of range" in str(e)


if __name__ == "__main__":
    lib_path, fn_name, out_path = sys.argv[1:4]
    lib = ctypes.CDLL(lib_path)
    lib.mcq_last_error.restype = ctypes.c_char_p
    np.savez_compressed(out_path, **pack(outcomes(getattr(lib, fn_name), lib.mcq_last_error)))
