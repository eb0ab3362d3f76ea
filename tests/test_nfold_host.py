"""CPU-only: the n-fold way in host code (mcq_nfold_host) against its NumPy restatement (tests/nfold_util.py) on every output, the
history included, at N = 2 .. 13, 16, 17, 24, 25, 31, 32 under rows from beta = 0 to beta = 8 and both clocks; the restatement's Philox
against the oracle's; the layout of the mcq_nfold block and the build's twelfth list; every refusal with its text; the third table of
bindings; a run cut at every segment boundary; an event counter that crosses 2^32; strict minima that sleep; the 4096 events of a step
under a clock of zeros; the mean of the clock's table; and the stationary distribution on a board small enough to enumerate."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

import mcq_amd
from tests import heatbath_util as hu
from tests import nfold_util as nu
from tests import quench_util as qu

abi = mcq_amd.abi
nfold = mcq_amd.nfold
quench = mcq_amd.quench
_lib = mcq_amd._lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BETAS = (0.0, 0.3, 1.0, 3.0, 8.0)  # from every weight 2^24 to a row whose d = 3 is already 0


def test_restatement_philox_equals_the_oracles():
    from oracle import oracle

    rs = np.random.RandomState(11)
    for _ in range(40):
        ctr = [int(rs.randint(0, 2**32, dtype=np.uint64)), int(rs.randint(1, 2**31, dtype=np.uint64)), 0, 0]  # a non-zero high word
        key = [int(rs.randint(0, 2**32, dtype=np.uint64)), nu.KEY_WORD]
        assert nu.philox(ctr, key) == [int(x) for x in oracle.philox_block(ctr, key)], (ctr, key)
    for ctr, key in (([0, 0, 0, 0], [0, 11]), ([2**32 - 1, 2**32 - 1, 0, 0], [2**32 - 1, 11]), ([1, 2, 3, 4], [5, 6])):
        assert nu.philox(ctr, key) == [int(x) for x in oracle.philox_block(ctr, key)], (ctr, key)
    e = (5 << 32) + 77  # block e: the two halves of e are counter words 0 and 1, key word 1 is 11
    assert nu.block(9, e) == [int(x) for x in oracle.philox_block([77, 5, 0, 0], [9, 11])]
    assert nu.block(9, e) != [int(x) for x in oracle.philox_block([77, 5, 0, 0], [9, 10])]  # not the stream of mcq_relink3d


def test_the_clock_reads_the_bits_below_the_leading_one():
    ln2, ct = nfold.clock_tables("exp")
    assert ln2 == round(2**24 * np.log(2)) and ct.dtype == np.uint32 and ct.shape == (256,)
    assert int(ct.max()) <= 1 << abi.NFOLD_CLOCK_BITS and ln2 <= 1 << 24
    assert nu.ell(0, ln2, ct) == 32 * ln2 + int(ct[0]) and nu.ell(1, ln2, ct) == 31 * ln2 + int(ct[0])
    assert nu.ell(3, ln2, ct) == 30 * ln2 + int(ct[128]) and nu.ell(0xFFFFFFFF, ln2, ct) == int(ct[255]) and nu.ell(0x80000000, ln2, ct) == int(ct[0])
    x = 0x00012345  # 17 significant bits: z = 15, the 8 bits below the leading one are 0x12345 >> 8 & 255 = 0x23
    assert nu.ell(x, ln2, ct) == 15 * ln2 + int(ct[0x23])
    mean = nfold.clock_tables("mean")
    assert mean[0] == 0 and (mean[1] == 1 << 24).all()
    with pytest.raises(ValueError, match="Unknown clock"):
        nfold.clock_tables("gamma")


def test_the_mean_of_the_clock_over_its_exact_distribution():
    """x is uniform over 2^32 words: z leading zeros and y below them are met by 2^(23 - z) words each up to z = 23, beyond it by one
    word for every y whose bits below the word's end are zero, and x = 0 is one word.  The mean of l is 2^24 to 1e-5."""
    ln2, ct = nfold.clock_tables("exp")
    total = nu.ell(0, ln2, ct)
    for z in range(32):
        p = 31 - z  # bits below the leading one
        for y in range(256):
            if p >= 8:
                count = 1 << (p - 8)
            else:
                count = 1 if y & ((1 << (8 - p)) - 1) == 0 else 0
            total += count * (z * ln2 + int(ct[y]))
    mean = total / 2**32 / 2**24
    print(f"mean of l / 2^24 = {mean:.9f}")
    assert abs(mean - 1) < 1e-5
    brute = sum(nu.ell(x, ln2, ct) for x in range(0, 2**32, 2**32 // 4096 + 1)) / len(range(0, 2**32, 2**32 // 4096 + 1)) / 2**24
    assert abs(brute - 1) < 0.05  # the restatement's l on a coarse grid of words: the same law


def test_weight_tables():
    t = nfold.weight_tables(BETAS)
    assert t.dtype == np.uint32 and t.shape == (5, abi.MAX_NFOLD_TABLE) and (t[0] == 1 << 24).all() and int(t.max()) == 1 << 24
    assert [int(v) for v in t[4][:4]] == [1 << 24, int(np.floor(2**24 * np.exp(-8.0))), int(np.floor(2**24 * np.exp(-16.0))), 0]
    assert nfold.weight_tables([8.0]).shape == (1, 4) and nfold.weight_tables([]).shape == (0, 1)
    with pytest.raises(ValueError, match="beta >= 0"):
        nfold.weight_tables([1.0, -0.1])


@pytest.mark.parametrize("N", tuple(range(2, 14)) + (16, 17, 24, 25, 31, 32))
def test_host_code_equals_the_restatement(N):
    n = 4 if N <= 13 else 2 if N <= 17 else 1
    steps = 6 if N <= 17 else 4
    tabs = nfold.weight_tables(BETAS)
    s = qu.random_boards(N, n, 100 + N, over=True)
    seeds = abi.seeds_for(4000000000 + N, n)
    met = np.zeros(3, dtype=np.int64)
    for clock in nfold.CLOCKS:
        got = nfold.nfold_states_host(N, s, seeds, tabs, steps, clock=clock, hist=True)
        assert got["state"].shape == got["best_state"].shape == (n, N * N) and got["energy_hist"].shape == (n, 6)
        assert got["need_out"].dtype == got["weight_out"].dtype == np.uint64 and got["best_step"].dtype == np.int64
        want = nu.nfold_many(N, s, seeds, tabs, steps, nfold.clock_tables(clock))
        nu.assert_equal(got, want, f"N = {N}, {clock}")
        met += [int(got["n_uphill"].sum()), int(got["n_flat"].sum()), int(got["events_out"].sum())]
        assert (got["best_energy"] <= got["energy_hist"].min(axis=1)).all() and (got["energy_hist"][:, -1] == got["energy_out"]).all()
        for r in range(n):
            assert qu.energy(N, got["state"][r]) == got["energy_out"][r] and qu.energy(N, got["best_state"][r]) == got["best_energy"][r]
    assert met[2] > 0 and (N == 2 or (met[2] > met[0] + met[1] and met[0] > 0 and met[1] > 0)), met  # downhill, uphill and flat events were compared
    # beta = 0 last: every weight is 2^24 and W = M 2^24, where U needs the whole 128-bit product (2^64 W at N = 32 is 2^103)
    got = nfold.nfold_states_host(N, s, seeds, tabs[::-1], steps, clock="exp")
    nu.assert_equal(got, nu.nfold_many(N, s, seeds, tabs[::-1], steps, nfold.clock_tables("exp")), f"N = {N}, beta = 0 last",
                    fields=nu.FIELDS)
    assert (got["weight_out"] == N * N * (N - 1) << 24).all()


def test_struct_layout_and_build():
    fields = [f for f, _ in abi.Nfold._fields_]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "mcq.h"\nint main(){printf("%zu %d %d %d %d %d %d %d", sizeof(mcq_nfold), MCQ_ABI_VERSION, ' \
        'MCQ_MAX_NFOLD_TABLE, MCQ_NFOLD_TIME_BITS, MCQ_NFOLD_WEIGHT_BITS, MCQ_NFOLD_CLOCK_BITS, MCQ_NFOLD_NEED_BITS, MCQ_NFOLD_STEP_BITS);' \
        + "".join(f'printf(" %zu", offsetof(mcq_nfold, {f}));' for f in fields) + "return 0;}"
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(prog)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")], check=True)
        out = subprocess.run([os.path.join(d, "t")], capture_output=True, text=True, check=True).stdout.split()
    assert int(out[0]) == ctypes.sizeof(abi.Nfold) and int(out[1]) == 6 == abi.ABI_VERSION
    assert [int(x) for x in out[2:8]] == [abi.MAX_NFOLD_TABLE, abi.NFOLD_TIME_BITS, abi.NFOLD_WEIGHT_BITS, abi.NFOLD_CLOCK_BITS, abi.NFOLD_NEED_BITS,
                                          abi.NFOLD_STEP_BITS] == [128, 12, 24, 26, 45, 50]
    assert [int(x) for x in out[8:]] == [getattr(abi.Nfold, f).offset for f in fields]
    assert set(abi.NFOLD_DTYPES) | {"state", "best_state"} == set(nu.FIELDS) | {"energy_hist"} == set(nfold.FIELDS)
    b = mcq_amd.build
    assert b.NFOLD_SOURCES == [os.path.join(b.CSRC, "mcq_nfold.hip")] and os.path.exists(b.NFOLD_SOURCES[0])
    assert not set(b.NFOLD_SOURCES) & set(b.SOURCES + b.ADDED_SOURCES + b.TEMPER_SOURCES + b.TEMPER3D_SOURCES + b.PAIRS_SOURCES + b.HOP_SOURCES + b.HOP3D_SOURCES
                                         + b.TABU_SOURCES + b.TABU3D_SOURCES + b.RELINK_SOURCES + b.RELINK3D_SOURCES)
    L = _lib.lib()
    for name in ("mcq_nfold_device", "mcq_nfold_host", "mcq_nfold_last_error"):
        assert hasattr(L, name), name


def test_the_third_table_of_bindings():
    L = _lib.lib()
    assert tuple(_lib.SAMPLER_FEATURES) == ("nfold",) and not set(_lib.SAMPLER_FEATURES) & (set(_lib.FEATURES) | set(_lib.MORE_FEATURES))
    assert _lib.every_feature() == _lib.all_features() + list(_lib.SAMPLER_FEATURES.values())
    assert _lib.all_features() == list(_lib.FEATURES.values()) + list(_lib.MORE_FEATURES.values())
    for feature, row in _lib.SAMPLER_FEATURES.items():
        last = getattr(L, f"mcq_{row.prefix}_last_error")
        assert last.restype is ctypes.c_char_p and isinstance(last(), bytes)
        assert issubclass(row.struct, ctypes.Structure) and getattr(abi, row.struct.__name__) is row.struct
        assert row.entries[:2] == (feature + "_host", feature + "_device")
        for name in row.entries:
            fn = getattr(L, "mcq_" + name)
            host = name.endswith("_host")
            assert fn.restype is ctypes.c_int and fn.argtypes[0] is ctypes.POINTER(row.struct), name
            assert list(fn.argtypes[1:]) == ([] if host else [ctypes.c_void_p]), name
            call = getattr(_lib, name)
            assert callable(call) and call.__name__ == name and "mcq_" + name in call.__doc__ and "abi." + row.struct.__name__ in call.__doc__
            assert call.__code__.co_varnames[: call.__code__.co_argcount] == (("q",) if host else ("q", "stream"))
            assert (fn(None) if host else fn(None, None)) == abi.EINVAL and b"NULL" in last()
    # a refusal is read from the feature's own buffer, and leaves its neighbours' texts alone
    neighbours = [getattr(L, f"mcq_{p}_last_error")() for p in ("relink3d", "relink", "heatbath")]
    for block, word in ((nfold._block(6, 0, 1, 1, 0, 4, 0), "n_chains"), (nfold._block(1, 4, 1, 1, 0, 4, 0), "N out of range")):
        with pytest.raises(ValueError) as e:
            _lib.nfold_host(block)
        assert word in str(e.value) and str(e.value) == L.mcq_nfold_last_error().decode()
    assert neighbours == [getattr(L, f"mcq_{p}_last_error")() for p in ("relink3d", "relink", "heatbath")]


def test_refusals_each_with_its_message():
    L = _lib.lib()
    N, n, S = 6, 4, 3
    buf, other, spare = (np.zeros((n, N * N), dtype=np.uint8) for _ in range(3))
    seeds = abi.seeds_for(1, n)
    tabs = nfold.weight_tables([0.5] * S)
    ln2, ct = nfold.clock_tables("exp")
    hist = np.zeros((n, S + 1), dtype=np.int32)
    need, events = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.int64)

    def block(**kw):
        q = nfold._block(N, n, S, 10, 0, tabs.shape[1], ln2)
        q.seeds, q.table, q.clock_table, q.state_in, q.state_out = seeds.ctypes.data, tabs.ctypes.data, ct.ctypes.data, buf.ctypes.data, other.ctypes.data
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    refused = ((dict(mode=abi.MODE_FULL3D), b"mode: the n-fold way runs boards only"), (dict(mode=7), b"mode"), (dict(N=1), b"N out of range [2, 32]: 1"),
               (dict(N=33), b"N out of range [2, 32]: 33"), (dict(n_chains=0), b"n_chains out of range"), (dict(n_chains=-1), b"n_chains"),
               (dict(n_chains=1 << 31), b"n_chains"), (dict(n_segs=-1), b"n_segs must be >= 0"), (dict(first_seg=-1), b"first_seg must be >= 0"),
               (dict(seg_steps=0), b"seg_steps out of range [1, 2^31]: 0"), (dict(seg_steps=(1 << 31) + 1), b"seg_steps out of range"),
               (dict(seg_steps=-5), b"seg_steps out of range"), (dict(first_seg=(1 << 50) // 10 - 2), b"must stay below 2^50"),
               (dict(first_seg=1 << 62), b"must stay below 2^50"), (dict(n_segs=1 << 50, seg_steps=1), b"must stay below 2^50"),
               (dict(table_len=0), b"table_len out of range [1, 128]: 0"), (dict(table_len=129), b"table_len out of range [1, 128]: 129"),
               (dict(clock_ln2=-1), b"clock_ln2 out of range"), (dict(clock_ln2=(1 << 24) + 1), b"clock_ln2 out of range"),
               (dict(seeds=None), b"seeds is required"), (dict(state_in=None), b"state_in is required"), (dict(state_out=None), b"state_out is required"),
               (dict(clock_table=None), b"clock_table is required"), (dict(table=None), b"table is required when n_segs > 0"),
               (dict(best_state=buf.ctypes.data), b"best_state must be distinct"), (dict(best_state=other.ctypes.data), b"best_state must be distinct"),
               (dict(energy_hist=hist.ctypes.data, hist_stride=S), b"hist_stride must be >= n_segs + 1 = 4"),
               (dict(energy_hist=hist.ctypes.data, hist_stride=0), b"hist_stride"))
    before = [getattr(L, f"mcq_{p}_last_error")() for p in ("relink3d", "relink", "tabu", "heatbath")]
    for kw, msg in refused:
        for fn in (L.mcq_nfold_host, lambda q: L.mcq_nfold_device(q, None)):  # refused before any launch: no GPU here
            assert fn(ctypes.byref(block(**kw))) == abi.EINVAL, kw
            assert msg in L.mcq_nfold_last_error(), (kw, L.mcq_nfold_last_error())
    assert before == [getattr(L, f"mcq_{p}_last_error")() for p in ("relink3d", "relink", "tabu", "heatbath")]  # the message is the call's own
    assert L.mcq_nfold_host(None) == abi.EINVAL and L.mcq_nfold_device(None, None) == abi.EINVAL and b"NULL" in L.mcq_nfold_last_error()
    # what only the host entry can look at: the entries
    big = tabs.copy()
    big[1, 2] = (1 << 24) + 1
    bad_clock = ct.copy()
    bad_clock[200] = (1 << 26) + 1
    bad_need, bad_events = np.array([0, 0, 1 << 45, 0], dtype=np.uint64), np.array([0, -1, 0, 0], dtype=np.int64)
    for kw, msg in ((dict(table=big.ctypes.data), b"table[1][2] = 16777217 exceeds 2^24"), (dict(clock_table=bad_clock.ctypes.data), b"clock_table[200]"),
                    (dict(need_in=bad_need.ctypes.data), b"need_in[2]"), (dict(events_in=bad_events.ctypes.data), b"events_in[1] must be >= 0")):
        assert L.mcq_nfold_host(ctypes.byref(block(**kw))) == abi.EINVAL and msg in L.mcq_nfold_last_error(), (kw, L.mcq_nfold_last_error())
    # at the bounds: accepted
    full = np.full((S, tabs.shape[1]), 1 << 24, dtype=np.uint32)
    assert L.mcq_nfold_host(ctypes.byref(block(table=full.ctypes.data, seg_steps=1))) == abi.OK
    assert L.mcq_nfold_host(ctypes.byref(block(n_segs=0, table=None))) == abi.OK  # a recount and a copy
    assert L.mcq_nfold_host(ctypes.byref(block(first_seg=(1 << 50) // 10 - 4))) == abi.OK
    assert L.mcq_nfold_host(ctypes.byref(block(energy_hist=hist.ctypes.data, hist_stride=S + 1))) == abi.OK
    assert L.mcq_nfold_host(ctypes.byref(block(hist_stride=0))) == abi.OK  # not read without energy_hist
    assert L.mcq_nfold_host(ctypes.byref(block(best_state=spare.ctypes.data, need_in=need.ctypes.data, events_in=events.ctypes.data))) == abi.OK
    assert L.mcq_nfold_host(ctypes.byref(block(state_out=buf.ctypes.data))) == abi.OK  # in place
    with pytest.raises(ValueError, match="N out of range"):
        nfold.nfold_states_host(33, np.zeros((2, 33 * 33), dtype=np.uint8), seeds[:2], tabs, 10)
    with pytest.raises(ValueError, match="n_chains"):
        nfold.nfold_states_host(6, np.zeros((0, 36), dtype=np.uint8), seeds[:0], tabs, 10)
    with pytest.raises(ValueError, match="seeds"):
        nfold.nfold_states_host(6, buf, seeds[:3], tabs, 10)
    with pytest.raises(ValueError, match="final_state layout"):
        nfold.nfold_states_host(6, np.zeros((2, 35), dtype=np.uint8), seeds[:2], tabs, 10)
    with pytest.raises(ValueError, match="need_in must have one entry per chain"):
        nfold.nfold_states_host(6, buf, seeds, tabs, 10, need_in=need[:2])
    with pytest.raises(ValueError, match=r"tables must be uint32\[n_segs\]\[table_len\]"):
        nfold.nfold_states_host(6, buf, seeds, tabs[0], 10)
    with pytest.raises(ValueError, match="multiple of seg_steps"):
        nfold.anneal_nfold(6, 1001, "random", {"type": "constant", "beta": 1.0}, seeds, seg_steps=10)
    with pytest.raises(ValueError, match="one schedule"):
        nfold.anneal_nfold(6, 1000, "random", [{"type": "constant", "beta": 1.0}], seeds, seg_steps=10)
    with pytest.raises(ValueError, match="Unknown clock"):
        nfold.anneal_nfold(6, 1000, "random", {"type": "constant", "beta": 1.0}, seeds, seg_steps=10, clock="tick")


def test_no_segment_is_a_recount_and_a_copy():
    N, n = 7, 5
    s = qu.random_boards(N, n, 3, over=True)
    ev = np.array([0, 5, 1 << 40, 7, 9], dtype=np.int64)
    got = nfold.nfold_states_host(N, s, abi.seeds_for(3, n), nfold.weight_tables([]), 10, events_in=ev, hist=True)
    want = nu.nfold_many(N, s, abi.seeds_for(3, n), nfold.weight_tables([]), 10, nfold.clock_tables("exp"), events_in=ev)
    nu.assert_equal(got, want, "no segment")
    assert (got["state"] == np.minimum(s, N - 1)).all() and (got["best_state"] == got["state"]).all() and (got["events_out"] == ev).all()
    assert (got["weight_out"] == 0).all() and (got["best_step"] == 0).all() and got["energy_hist"].shape == (n, 1)
    assert [int(e) for e in got["energy_in"]] == [qu.energy(N, b) for b in s]


@pytest.mark.parametrize("N,clock", ((5, "exp"), (9, "mean"), (13, "exp")))
def test_a_run_cut_at_every_segment_boundary_is_the_unbroken_run(N, clock):
    n, S, steps = 6, 5, 25
    s = qu.random_boards(N, n, 60 + N)
    seeds = abi.seeds_for(900 + N, n)
    tabs = nfold.weight_tables(np.linspace(0.4, 2.5, S))
    whole = nfold.nfold_states_host(N, s, seeds, tabs, steps, clock=clock, hist=True)
    assert int(whole["events_out"].min()) > S  # events in every piece
    for cut in range(S + 1):
        a = nfold.nfold_states_host(N, s, seeds, tabs[:cut], steps, clock=clock, hist=True)
        b = nfold.nfold_states_host(N, a["state"], seeds, tabs[cut:], steps, first_seg=cut, clock=clock, need_in=a["need_out"], events_in=a["events_out"],
                                    hist=True)
        for k in ("state", "energy_out", "events_out", "need_out"):
            np.testing.assert_array_equal(b[k], whole[k], err_msg=f"cut {cut}: {k}")
        if cut < S:
            np.testing.assert_array_equal(b["weight_out"], whole["weight_out"])
        np.testing.assert_array_equal(np.concatenate([a["energy_hist"], b["energy_hist"][:, 1:]], axis=1), whole["energy_hist"])
        np.testing.assert_array_equal(a["n_uphill"] + b["n_uphill"], whole["n_uphill"])
        np.testing.assert_array_equal(a["n_flat"] + b["n_flat"], whole["n_flat"])
        # the first piece with the smallest best_energy holds the best of the whole, its step moved by the steps before the piece
        first = a["best_energy"] <= b["best_energy"]
        np.testing.assert_array_equal(np.where(first, a["best_energy"], b["best_energy"]), whole["best_energy"])
        np.testing.assert_array_equal(np.where(first, a["best_step"], b["best_step"] + cut * steps), whole["best_step"])
        np.testing.assert_array_equal(np.where(first[:, None], a["best_state"], b["best_state"]), whole["best_state"])
    # without the carried need the second piece is another run: the need is part of the chain
    a = nfold.nfold_states_host(N, s, seeds, tabs[:2], steps, clock=clock)
    b = nfold.nfold_states_host(N, a["state"], seeds, tabs[2:], steps, first_seg=2, clock=clock, events_in=a["events_out"])
    assert clock == "mean" or (b["need_out"] != whole["need_out"]).any()


def test_the_event_counter_carries_into_the_high_counter_word():
    N, n = 6, 4
    s = qu.random_boards(N, n, 8)
    seeds = abi.seeds_for(77, n)
    tabs = nfold.weight_tables([0.5, 1.0])
    ev = np.full(n, 2**32 - 3, dtype=np.int64)
    got = nfold.nfold_states_host(N, s, seeds, tabs, 20, events_in=ev, hist=True)
    assert int(got["events_out"].min()) > 2**32 + 2
    nu.assert_equal(got, nu.nfold_many(N, s, seeds, tabs, 20, nfold.clock_tables("exp"), events_in=ev), "events_in = 2^32 - 3")
    low = nfold.nfold_states_host(N, s, seeds, tabs, 20, events_in=ev - 2**32 + 2**31)  # a counter that wrapped at 32 bits would agree with another run
    assert (low["state"] != got["state"]).any()
    assert nu.block(5, 2**32) == nu.philox((0, 1, 0, 0), (5, 11)) != nu.block(5, 0)


def _strict_minima(N, n, seed):
    """Placements behind the pair-move quench with W = 0 under T = [2^24, 0]: no single move keeps or lowers E."""
    q = quench.quench_pairs_host(N, qu.random_boards(N, n, seed), conflicts=False)["state"]
    row = np.array([[1 << 24, 0]], dtype=np.uint32)
    w = nfold.nfold_states_host(N, q, abi.seeds_for(1, n), row, 1)["weight_out"]
    return q[w == 0], row


@pytest.mark.parametrize("N", (5, 7))
def test_a_strict_minimum_sleeps_and_keeps_its_need(N):
    m, row = _strict_minima(N, 400, N)
    print(f"N = {N}: {len(m)} of 400 quenched placements are strict minima")
    assert len(m) >= 3
    m = m[:16]
    n = len(m)
    need = (np.arange(n, dtype=np.uint64) * 12345 + 1) << 20
    ev = np.arange(n, dtype=np.int64) + 2**33
    got = nfold.nfold_states_host(N, m, abi.seeds_for(5, n), np.repeat(row, 3, axis=0), 1 << 31, need_in=need, events_in=ev, hist=True)
    np.testing.assert_array_equal(got["need_out"], need)
    np.testing.assert_array_equal(got["events_out"], ev)
    np.testing.assert_array_equal(got["state"], m)
    assert (got["weight_out"] == 0).all() and (got["n_uphill"] == 0).all() and (got["energy_hist"] == got["energy_in"][:, None]).all()
    nu.assert_equal(got, nu.nfold_many(N, m, abi.seeds_for(5, n), np.repeat(row, 3, axis=0), 1 << 31, nfold.clock_tables("exp"), need_in=need, events_in=ev),
                    "sleeping minima")
    # a row that lets them rise wakes them
    woken = nfold.nfold_states_host(N, m, abi.seeds_for(5, n), nfold.weight_tables([0.5]), 1000, need_in=need, events_in=ev)
    assert (woken["events_out"] > ev).all() and (woken["n_uphill"] > 0).all()


def test_a_clock_of_zeros_fires_4096_events_per_step():
    N, n, S = 3, 5, 2
    s = qu.random_boards(N, n, 12)
    seeds = abi.seeds_for(31, n)
    tabs = nfold.weight_tables([0.0] * S)  # every weight 2^24: W > 0 whatever the placement is
    zero = (0, np.zeros(256, dtype=np.uint32))
    got = nfold.nfold_states_host(N, s, seeds, tabs, 1, clock=zero, hist=True)
    assert (got["events_out"] == S << abi.NFOLD_TIME_BITS).all() and (got["need_out"] == 0).all()
    assert (got["best_step"] <= S).all() and (got["weight_out"] == N * N * (N - 1) << 24).all()
    nu.assert_equal({k: v[:2] for k, v in got.items()}, nu.nfold_many(N, s[:2], seeds[:2], tabs, 1, zero), "a clock of zeros")


def _wilson_hilferty(df, z=3.090232306167813):  # the 99.9 % quantile of chi^2 with df degrees of freedom
    return df * (1 - 2 / (9 * df) + z * np.sqrt(2 / (9 * df))) ** 3


@pytest.mark.parametrize("clock", nfold.CLOCKS)
@pytest.mark.parametrize("beta", (0.5, 1.0, 2.0))
def test_stationary_distribution_is_boltzmann(beta, clock):
    """N = 3: the histogram of energy_out of 8 192 chains from random boards after one segment of 300 Metropolis steps at constant beta
    against the exact Boltzmann weights of all 3^9 placements, for three seed bases and both clocks.  Bins of expected count < 5 are
    merged; chi^2 must stay below its 99.9 % quantile.  Seeded, hence deterministic: a failure is a finding about the rule or its
    implementation.  (A NumPy prototype of the rule with whole-step time, no fractional bits, fails this at 65 536 chains: the clock has
    12 fractional bits for that reason.)
    Measured with the Philox stream, chi^2 (degrees of freedom; bound), seed bases 42, 100000, 4000000000:
      beta 0.5 (12; 32.91): exp 6.25, 12.94, 16.48; mean 12.81, 12.41, 9.50
      beta 1.0 (9; 27.88): exp 10.03, 9.26, 3.74; mean 6.27, 10.80, 5.39
      beta 2.0 (5; 20.52): exp 3.83, 4.86, 4.24; mean 2.51, 5.15, 6.84"""
    N, n, steps = 3, 8192, 300
    exact = hu.boltzmann_energy_distribution(N, beta)
    assert abs(sum(exact.values()) - 1) < 1e-12
    try:
        from scipy.stats import chi2

        quantile = lambda df: float(chi2.ppf(0.999, df))  # noqa: E731
    except ImportError:
        quantile = _wilson_hilferty
    tabs = nfold.weight_tables([beta])
    for base in (42, 100000, 4000000000):
        s = qu.random_boards(N, n, base % 1000)
        got = nfold.nfold_states_host(N, s, abi.seeds_for(base, n), tabs, steps, clock=clock)
        energies = sorted(exact)
        expected = np.array([exact[e] * n for e in energies])
        observed = np.array([int((got["energy_out"] == e).sum()) for e in energies], dtype=np.float64)
        assert observed.sum() == n, "an energy that no placement has"
        exp_m, obs_m, ea, oa = [], [], 0.0, 0.0
        for e, o in zip(expected, observed):  # merge neighbours until every bin expects at least 5
            ea, oa = ea + e, oa + o
            if ea >= 5:
                exp_m.append(ea), obs_m.append(oa)
                ea = oa = 0.0
        if ea > 0:
            exp_m[-1] += ea
            obs_m[-1] += oa
        exp_m, obs_m = np.array(exp_m), np.array(obs_m)
        chi = float(((obs_m - exp_m) ** 2 / exp_m).sum())
        df = len(exp_m) - 1
        print(f"beta={beta} {clock} seeds {base}+: chi^2 = {chi:.2f} with {df} degrees of freedom, bound {quantile(df):.2f}")
        assert chi < quantile(df), f"beta={beta}, {clock}, seeds {base}+: chi^2 = {chi:.2f} >= {quantile(df):.2f} ({df} degrees of freedom)"
