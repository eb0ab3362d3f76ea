"""CPU-only: the full_3d n-fold way in host code (mcq_nfold3d_host) against its NumPy restatement (tests/nfold3d_util.py) on every
output, the history included, at N = 2 .. 6 with Q = 2, N^2 and N^3 - 1 and at N = 12, 13, 19, 20, 32 with few queens, under rows from
beta = 0 to beta = 8 and both clocks; the restatement's Philox against the oracle's; the layout of the mcq_nfold3d block, the LDS
formula and the build's thirteenth list; the fourth table of bindings; every refusal with its text; no segment; a run cut at every
segment boundary; an event counter that crosses 2^32; a row of zeros that sleeps; the 4096 events of a step under a clock of zeros; the
repeated-placement flag; the two cases of wide arithmetic against Python integers; and the stationary distribution on a cube small
enough to enumerate."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

import mcq_amd
from tests import heatbath3d_util as h3
from tests import nfold3d_util as n3
from tests import quench3d_util as q3

abi = mcq_amd.abi
nfold = mcq_amd.nfold
_lib = mcq_amd._lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BETAS = (0.0, 0.3, 1.0, 3.0, 8.0)  # from every weight 2^24 to a row whose d = 3 is already 0
FEW = {12: 40, 13: 17, 19: 23, 20: 31, 32: 5}
SHAPES = tuple((N, Q) for N in range(2, 7) for Q in sorted({2, N * N, N ** 3 - 1})) + tuple(FEW.items())


def _tables(betas=BETAS):
    return nfold.weight_tables(betas, abi.MAX_NFOLD3D_TABLE)


def test_restatement_philox_equals_the_oracles():
    from oracle import oracle

    rs = np.random.RandomState(12)
    for _ in range(40):
        ctr = [int(rs.randint(0, 2**32, dtype=np.uint64)), int(rs.randint(1, 2**31, dtype=np.uint64)), 0, 0]  # a non-zero high word
        key = [int(rs.randint(0, 2**32, dtype=np.uint64)), n3.KEY_WORD]
        assert n3.philox(ctr, key) == [int(x) for x in oracle.philox_block(ctr, key)], (ctr, key)
    assert n3.KEY_WORD == 12
    e = (5 << 32) + 77  # block e: the two halves of e are counter words 0 and 1, key word 1 is 12
    assert n3.block(9, e) == [int(x) for x in oracle.philox_block([77, 5, 0, 0], [9, 12])]
    assert n3.block(9, e) != [int(x) for x in oracle.philox_block([77, 5, 0, 0], [9, 11])]  # not the stream of mcq_nfold
    assert n3.block(9, e) != [int(x) for x in oracle.philox_block([77, 5, 0, 0], [9, 10])]  # nor that of mcq_relink3d
    header = open(os.path.join(ROOT, "include", "mcq.h")).read()
    assert "12 is this block's" in header and "13 is this block's" not in header  # the next free key word


def test_weight_tables_to_the_width_of_the_cube():
    t = _tables()
    assert t.dtype == np.uint32 and t.shape == (5, abi.MAX_NFOLD3D_TABLE) and (t[0] == 1 << 24).all() and int(t.max()) == 1 << 24
    assert nfold.weight_tables(BETAS).shape == (5, abi.MAX_NFOLD_TABLE)  # the default stays the boards'
    np.testing.assert_array_equal(t[:, : abi.MAX_NFOLD_TABLE], nfold.weight_tables(BETAS))
    assert nfold.weight_tables([8.0], abi.MAX_NFOLD3D_TABLE).shape == (1, 4)


def _inputs(N, Q):
    """(placements with bytes >= N, seeds, steps per segment) of the comparison at (N, Q)."""
    n = 3 if N <= 13 else 2
    return q3.random_placements(N, n, 100 + N + Q, Q=Q, over=True), abi.seeds_for(4000000000 + N + Q, n), 6 if N <= 6 else 3


@pytest.mark.parametrize("N,Q", SHAPES)
def test_host_code_equals_the_restatement(N, Q):
    s, seeds, steps = _inputs(N, Q)
    n, tabs = len(s), _tables()
    met = np.zeros(3, dtype=np.int64)
    for clock in nfold.CLOCKS:
        got = nfold.nfold_queens_host(N, s, seeds, tabs, steps, Q=Q, clock=clock, hist=True)
        assert got["state"].shape == got["best_state"].shape == (n, 3 * Q) and got["energy_hist"].shape == (n, 6)
        assert got["need_out"].dtype == got["weight_out"].dtype == np.uint64 and got["best_step"].dtype == np.int64 and got["flags"].dtype == np.int32
        want = n3.nfold_many(N, s, seeds, tabs, steps, nfold.clock_tables(clock), Q=Q)
        n3.assert_equal(got, want, f"N = {N}, Q = {Q}, {clock}")
        met += [int(got["n_uphill"].sum()), int(got["n_flat"].sum()), int(got["events_out"].sum())]
        assert (got["best_energy"] <= got["energy_hist"].min(axis=1)).all() and (got["energy_hist"][:, -1] == got["energy_out"]).all()
        for r in range(n):
            assert q3.energy(N, got["state"][r]) == got["energy_out"][r] and q3.energy(N, got["best_state"][r]) == got["best_energy"][r]
    assert met[2] > 0, met
    # beta = 0 last: every weight is 2^24 and W = M 2^24, where U needs the whole 128-bit product
    got = nfold.nfold_queens_host(N, s, seeds, tabs[::-1], steps, Q=Q, clock="exp")
    n3.assert_equal(got, n3.nfold_many(N, s, seeds, tabs[::-1], steps, nfold.clock_tables("exp"), Q=Q), f"N = {N}, Q = {Q}, beta = 0 last", fields=n3.FIELDS)
    assert (got["weight_out"] == Q * (N ** 3 - Q) << 24).all()


def test_downhill_flat_and_uphill_events_were_all_compared():
    """From the host code's outputs on the inputs of the comparisons above (N = 2 has one energy per Q: flat moves only)."""
    for N in sorted({N for N, _ in SHAPES} - {2}):
        up = flat = events = 0
        for Q in (Q for n, Q in SHAPES if n == N):
            s, seeds, steps = _inputs(N, Q)
            for clock in nfold.CLOCKS:
                got = nfold.nfold_queens_host(N, s, seeds, _tables(), steps, Q=Q, clock=clock)
                up, flat, events = up + int(got["n_uphill"].sum()), flat + int(got["n_flat"].sum()), events + int(got["events_out"].sum())
        print(f"N = {N}: {events} events, {up} uphill, {flat} flat")
        assert up > 0 and flat > 0 and events > up + flat, (N, up, flat, events)


def test_struct_layout_lds_formula_and_build():
    fields = [f for f, _ in abi.Nfold3d._fields_]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "mcq.h"\nint main(){printf("%zu %d %d %d %d %d %d", sizeof(mcq_nfold3d), MCQ_ABI_VERSION, ' \
        'MCQ_MAX_NFOLD3D_TABLE, MCQ_NFOLD3D_NEED_BITS, MCQ_MAX_NFOLD3D_LDS, MCQ_NFOLD3D_REPEATED, MCQ_MAX_HEATBATH_TABLE);' \
        + "".join(f'printf(" %zu", offsetof(mcq_nfold3d, {f}));' for f in fields) + "return 0;}"
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(prog)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")], check=True)
        out = subprocess.run([os.path.join(d, "t")], capture_output=True, text=True, check=True).stdout.split()
    assert int(out[0]) == ctypes.sizeof(abi.Nfold3d) and int(out[1]) == 6 == abi.ABI_VERSION
    assert [int(x) for x in out[2:7]] == [abi.MAX_NFOLD3D_TABLE, abi.NFOLD3D_NEED_BITS, abi.MAX_NFOLD3D_LDS, abi.NFOLD3D_REPEATED, abi.MAX_HEATBATH_TABLE] \
        == [512, 58, 160 * 1024, 1, 512]
    assert [int(x) for x in out[7:]] == [getattr(abi.Nfold3d, f).offset for f in fields]
    assert set(abi.NFOLD3D_DTYPES) | {"state", "best_state"} == set(n3.FIELDS) | {"energy_hist"} == set(nfold.FIELDS_3D)
    # need = M l(x2) stays below 2^58: M <= 2^28 at N = 32 and l < 32 2^24 + 2^26
    assert (32 ** 3 // 2) ** 2 * (32 * (1 << 24) + (1 << 26)) < 1 << abi.NFOLD3D_NEED_BITS
    # the LDS of a chain: 2 376 dwords, R, the field, occ, the queens
    assert abi.nfold3d_lds_bytes(32) == abi.nfold3d_lds_bytes(32, 1024) == 89376 and abi.nfold3d_lds_bytes(12) == 4 * (2376 + 288 + 432 + 54 + 72)
    assert all(abi.nfold3d_lds_bytes(N) <= abi.MAX_NFOLD3D_LDS for N in range(2, 33))
    assert n3.largest_queens(abi, 32) == 8470 and abi.nfold3d_lds_bytes(20, 7999) <= abi.MAX_NFOLD3D_LDS
    b = mcq_amd.build
    assert b.NFOLD3D_SOURCES == [os.path.join(b.CSRC, "mcq_nfold3d.hip")] and os.path.exists(b.NFOLD3D_SOURCES[0])
    assert not set(b.NFOLD3D_SOURCES) & set(b.SOURCES + b.ADDED_SOURCES + b.TEMPER_SOURCES + b.TEMPER3D_SOURCES + b.PAIRS_SOURCES + b.HOP_SOURCES + b.HOP3D_SOURCES
                                           + b.TABU_SOURCES + b.TABU3D_SOURCES + b.RELINK_SOURCES + b.RELINK3D_SOURCES + b.NFOLD_SOURCES)
    L = _lib.lib()
    for name in ("mcq_nfold3d_device", "mcq_nfold3d_host", "mcq_nfold3d_last_error"):
        assert hasattr(L, name), name


def test_the_fourth_table_of_bindings():
    L = _lib.lib()
    assert tuple(_lib.SAMPLER3D_FEATURES) == ("nfold3d",)
    assert not set(_lib.SAMPLER3D_FEATURES) & (set(_lib.FEATURES) | set(_lib.MORE_FEATURES) | set(_lib.SAMPLER_FEATURES))
    assert _lib.bound_features() == _lib.every_feature() + list(_lib.SAMPLER3D_FEATURES.values())
    assert _lib.every_feature() == _lib.all_features() + list(_lib.SAMPLER_FEATURES.values())
    assert _lib.SAMPLER3D_FEATURES["nfold3d"] == _lib.Feature(abi.Nfold3d, "nfold3d", ("nfold3d_host", "nfold3d_device"))
    for feature, row in _lib.SAMPLER3D_FEATURES.items():
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
    neighbours = [getattr(L, f"mcq_{p}_last_error")() for p in ("nfold", "relink3d", "tabu3d", "heatbath3d")]
    for block, word in ((nfold._block3d(6, 0, 0, 1, 1, 0, 4, 0), "n_chains"), (nfold._block3d(1, 0, 4, 1, 1, 0, 4, 0), "N out of range")):
        with pytest.raises(ValueError) as e:
            _lib.nfold3d_host(block)
        assert word in str(e.value) and str(e.value) == L.mcq_nfold3d_last_error().decode()
    assert neighbours == [getattr(L, f"mcq_{p}_last_error")() for p in ("nfold", "relink3d", "tabu3d", "heatbath3d")]
    # and the board form keeps refusing full_3d in its own words
    q = nfold._block(6, 4, 1, 1, 0, 4, 0)
    q.mode = abi.MODE_FULL3D
    assert L.mcq_nfold_host(ctypes.byref(q)) == abi.EINVAL and b"boards only" in L.mcq_nfold_last_error()
    assert b"boards only" not in L.mcq_nfold3d_last_error()


def test_refusals_each_with_its_message():
    L = _lib.lib()
    N, Q, n, S = 6, 36, 4, 3
    buf, other, spare = (np.zeros((n, 3 * Q), dtype=np.uint8) for _ in range(3))
    for a in (buf, other, spare):
        a[:] = q3.random_placements(N, n, 1, Q=Q)
    seeds = abi.seeds_for(1, n)
    tabs = _tables([0.5] * S)
    ln2, ct = nfold.clock_tables("exp")
    hist = np.zeros((n, S + 1), dtype=np.int32)
    need, events = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.int64)

    def block(**kw):
        q = nfold._block3d(N, 0, n, S, 10, 0, tabs.shape[1], ln2)
        q.seeds, q.table, q.clock_table, q.state_in, q.state_out = seeds.ctypes.data, tabs.ctypes.data, ct.ctypes.data, buf.ctypes.data, other.ctypes.data
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    refused = ((dict(mode=abi.MODE_BOARD), b"mode: mcq_nfold3d runs full_3d placements only"), (dict(mode=7), b"mode"), (dict(N=1), b"N out of range [2, 32]: 1"),
               (dict(N=33), b"N out of range [2, 32]: 33 (the full_3d n-fold way stops at N = 32"), (dict(N=65), b"N out of range [2, 32]: 65"),
               (dict(n_queens=1), b"n_queens out of range [2, N^3 - 1 = 215] (0 = N^2): 1"), (dict(n_queens=216), b"n_queens out of range [2, N^3 - 1 = 215]"),
               (dict(n_queens=-3), b"n_queens out of range"),
               (dict(n_chains=0), b"n_chains out of range"), (dict(n_chains=-1), b"n_chains"),
               (dict(n_chains=1 << 31), b"n_chains"), (dict(n_segs=-1), b"n_segs must be >= 0"), (dict(first_seg=-1), b"first_seg must be >= 0"),
               (dict(seg_steps=0), b"seg_steps out of range [1, 2^31]: 0"), (dict(seg_steps=(1 << 31) + 1), b"seg_steps out of range"),
               (dict(seg_steps=-5), b"seg_steps out of range"), (dict(first_seg=(1 << 50) // 10 - 2), b"must stay below 2^50"),
               (dict(first_seg=1 << 62), b"must stay below 2^50"), (dict(n_segs=1 << 50, seg_steps=1), b"must stay below 2^50"),
               (dict(table_len=0), b"table_len out of range [1, 512]: 0"), (dict(table_len=513), b"table_len out of range [1, 512]: 513"),
               (dict(clock_ln2=-1), b"clock_ln2 out of range"), (dict(clock_ln2=(1 << 24) + 1), b"clock_ln2 out of range"),
               (dict(seeds=None), b"seeds is required"), (dict(state_in=None), b"state_in is required"), (dict(state_out=None), b"state_out is required"),
               (dict(clock_table=None), b"clock_table is required"), (dict(table=None), b"table is required when n_segs > 0"),
               (dict(best_state=buf.ctypes.data), b"best_state must be distinct"), (dict(best_state=other.ctypes.data), b"best_state must be distinct"),
               (dict(energy_hist=hist.ctypes.data, hist_stride=S), b"hist_stride must be >= n_segs + 1 = 4"),
               (dict(energy_hist=hist.ctypes.data, hist_stride=0), b"hist_stride"))
    before = [getattr(L, f"mcq_{p}_last_error")() for p in ("nfold", "relink3d", "tabu3d", "heatbath")]
    for kw, msg in refused:
        for fn in (L.mcq_nfold3d_host, lambda q: L.mcq_nfold3d_device(q, None)):  # refused before any launch: no GPU here
            assert fn(ctypes.byref(block(**kw))) == abi.EINVAL, kw
            assert msg in L.mcq_nfold3d_last_error(), (kw, L.mcq_nfold3d_last_error())
    assert before == [getattr(L, f"mcq_{p}_last_error")() for p in ("nfold", "relink3d", "tabu3d", "heatbath")]  # the message is the call's own
    assert L.mcq_nfold3d_host(None) == abi.EINVAL and L.mcq_nfold3d_device(None, None) == abi.EINVAL and b"NULL" in L.mcq_nfold3d_last_error()
    # the device entry alone: a chain above the LDS of a workgroup, with N, Q and the bytes in its text
    big = n3.largest_queens(abi, 32) + 1
    assert L.mcq_nfold3d_device(ctypes.byref(block(N=32, n_queens=big)), None) == abi.EINVAL
    assert f"N = 32 with n_queens = {big}: a chain takes {abi.nfold3d_lds_bytes(32, big)} bytes of LDS, above the 163840".encode() in L.mcq_nfold3d_last_error()
    # what only the host entry can look at: the entries
    high = tabs.copy()
    high[1, 2] = (1 << 24) + 1
    bad_clock = ct.copy()
    bad_clock[200] = (1 << 26) + 1
    bad_need, bad_events = np.array([0, 0, 1 << 58, 0], dtype=np.uint64), np.array([0, -1, 0, 0], dtype=np.int64)
    for kw, msg in ((dict(table=high.ctypes.data), b"table[1][2] = 16777217 exceeds 2^24"), (dict(clock_table=bad_clock.ctypes.data), b"clock_table[200]"),
                    (dict(need_in=bad_need.ctypes.data), b"need_in[2] = 288230376151711744 is not below 2^58"),
                    (dict(events_in=bad_events.ctypes.data), b"events_in[1] must be >= 0")):
        assert L.mcq_nfold3d_host(ctypes.byref(block(**kw))) == abi.EINVAL and msg in L.mcq_nfold3d_last_error(), (kw, L.mcq_nfold3d_last_error())
    # at the bounds: accepted
    full = np.full((S, tabs.shape[1]), 1 << 24, dtype=np.uint32)
    ok_need = np.full(n, (1 << 58) - 1, dtype=np.uint64)
    assert L.mcq_nfold3d_host(ctypes.byref(block(table=full.ctypes.data, seg_steps=1))) == abi.OK
    assert L.mcq_nfold3d_host(ctypes.byref(block(n_segs=0, table=None))) == abi.OK  # a recount and a copy
    assert L.mcq_nfold3d_host(ctypes.byref(block(first_seg=(1 << 50) // 10 - 4))) == abi.OK
    assert L.mcq_nfold3d_host(ctypes.byref(block(energy_hist=hist.ctypes.data, hist_stride=S + 1))) == abi.OK
    assert L.mcq_nfold3d_host(ctypes.byref(block(hist_stride=0))) == abi.OK  # not read without energy_hist
    assert L.mcq_nfold3d_host(ctypes.byref(block(best_state=spare.ctypes.data, need_in=ok_need.ctypes.data, events_in=events.ctypes.data))) == abi.OK
    assert L.mcq_nfold3d_host(ctypes.byref(block(state_out=buf.ctypes.data))) == abi.OK  # in place
    assert L.mcq_nfold3d_host(ctypes.byref(block(n_queens=2))) == abi.OK and L.mcq_nfold3d_host(ctypes.byref(block(n_queens=36))) == abi.OK
    with pytest.raises(ValueError, match="N out of range"):
        nfold.nfold_queens_host(33, np.zeros((2, 3 * 33 * 33), dtype=np.uint8), seeds[:2], tabs, 10)
    with pytest.raises(ValueError, match="n_chains"):
        nfold.nfold_queens_host(6, np.zeros((0, 108), dtype=np.uint8), seeds[:0], tabs, 10)
    with pytest.raises(ValueError, match="seeds"):
        nfold.nfold_queens_host(6, buf, seeds[:3], tabs, 10)
    with pytest.raises(ValueError, match="final_state layout of full_3d"):
        nfold.nfold_queens_host(6, np.zeros((2, 107), dtype=np.uint8), seeds[:2], tabs, 10)
    with pytest.raises(ValueError, match="need_in must have one entry per chain"):
        nfold.nfold_queens_host(6, buf, seeds, tabs, 10, need_in=need[:2])
    with pytest.raises(ValueError, match=r"tables must be uint32\[n_segs\]\[table_len\]"):
        nfold.nfold_queens_host(6, buf, seeds, tabs[0], 10)
    with pytest.raises(ValueError, match="Unknown mcmc_type"):
        nfold.anneal_nfold(6, 1000, "random", {"type": "constant", "beta_const": 1.0}, seeds, seg_steps=10, mcmc_type="cube")
    with pytest.raises(ValueError, match="multiple of seg_steps"):
        nfold.anneal_nfold(6, 1001, "random", {"type": "constant", "beta_const": 1.0}, seeds, seg_steps=10, mcmc_type="full_3d")
    with pytest.raises(ValueError, match="n_queens out of range"):
        nfold.anneal_nfold(6, 1000, "random", {"type": "constant", "beta_const": 1.0}, seeds, seg_steps=10, mcmc_type="full_3d", Q=216)


def test_no_segment_is_a_recount_and_a_copy():
    N, Q, n = 7, 30, 5
    s = q3.random_placements(N, n, 3, Q=Q, over=True)
    ev = np.array([0, 5, 1 << 40, 7, 9], dtype=np.int64)
    none = nfold.weight_tables([])
    got = nfold.nfold_queens_host(N, s, abi.seeds_for(3, n), none, 10, Q=Q, events_in=ev, hist=True)
    want = n3.nfold_many(N, s, abi.seeds_for(3, n), none, 10, nfold.clock_tables("exp"), Q=Q, events_in=ev)
    n3.assert_equal(got, want, "no segment")
    assert (got["state"] == np.minimum(s, N - 1)).all() and (got["best_state"] == got["state"]).all() and (got["events_out"] == ev).all()
    assert (got["weight_out"] == 0).all() and (got["best_step"] == 0).all() and got["energy_hist"].shape == (n, 1) and (got["flags"] == 0).all()
    assert [int(e) for e in got["energy_in"]] == [q3.pairwise_energy(N, b) for b in s]


@pytest.mark.parametrize("N,Q,clock", ((4, 16, "exp"), (6, 50, "mean"), (13, 19, "exp")))
def test_a_run_cut_at_every_segment_boundary_is_the_unbroken_run(N, Q, clock):
    n, S, steps = 6, 5, 25
    s = q3.random_placements(N, n, 60 + N, Q=Q)
    seeds = abi.seeds_for(900 + N, n)
    tabs = _tables(np.linspace(0.4, 2.5, S))
    kw = dict(Q=Q, clock=clock, hist=True)
    whole = nfold.nfold_queens_host(N, s, seeds, tabs, steps, **kw)
    assert int(whole["events_out"].min()) > S  # events in every piece
    for cut in range(S + 1):
        a = nfold.nfold_queens_host(N, s, seeds, tabs[:cut], steps, **kw)
        b = nfold.nfold_queens_host(N, a["state"], seeds, tabs[cut:], steps, first_seg=cut, need_in=a["need_out"], events_in=a["events_out"], **kw)
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
    a = nfold.nfold_queens_host(N, s, seeds, tabs[:2], steps, Q=Q, clock=clock)
    b = nfold.nfold_queens_host(N, a["state"], seeds, tabs[2:], steps, Q=Q, first_seg=2, clock=clock, events_in=a["events_out"])
    assert clock == "mean" or (b["need_out"] != whole["need_out"]).any()


def test_the_event_counter_carries_into_the_high_counter_word():
    N, Q, n = 5, 12, 4
    s = q3.random_placements(N, n, 8, Q=Q)
    seeds = abi.seeds_for(77, n)
    tabs = _tables([0.5, 1.0])
    ev = np.full(n, 2**32 - 3, dtype=np.int64)
    got = nfold.nfold_queens_host(N, s, seeds, tabs, 20, Q=Q, events_in=ev, hist=True)
    assert int(got["events_out"].min()) > 2**32 + 2
    n3.assert_equal(got, n3.nfold_many(N, s, seeds, tabs, 20, nfold.clock_tables("exp"), Q=Q, events_in=ev), "events_in = 2^32 - 3")
    low = nfold.nfold_queens_host(N, s, seeds, tabs, 20, Q=Q, events_in=ev - 2**32 + 2**31)  # a counter that wrapped at 32 bits would agree with another run
    assert (low["state"] != got["state"]).any()
    assert n3.block(5, 2**32) == n3.philox((0, 1, 0, 0), (5, 12)) != n3.block(5, 0)


def test_a_row_of_zeros_sleeps_and_keeps_its_need_and_state():
    N, Q, n = 6, 20, 7
    s = q3.random_placements(N, n, 6, Q=Q)
    rows = np.zeros((3, 4), dtype=np.uint32)
    need = (np.arange(n, dtype=np.uint64) * 12345 + 1) << 33
    ev = np.arange(n, dtype=np.int64) + 2**33
    got = nfold.nfold_queens_host(N, s, abi.seeds_for(5, n), rows, 1 << 31, Q=Q, need_in=need, events_in=ev, hist=True)
    np.testing.assert_array_equal(got["need_out"], need)
    np.testing.assert_array_equal(got["events_out"], ev)
    np.testing.assert_array_equal(got["state"], s)
    assert (got["weight_out"] == 0).all() and (got["n_uphill"] == 0).all() and (got["energy_hist"] == got["energy_in"][:, None]).all()
    n3.assert_equal(got, n3.nfold_many(N, s, abi.seeds_for(5, n), rows, 1 << 31, nfold.clock_tables("exp"), Q=Q, need_in=need, events_in=ev), "a row of zeros")
    # a row that lets them move wakes them
    woken = nfold.nfold_queens_host(N, s, abi.seeds_for(5, n), _tables([0.5]), 1000, Q=Q, need_in=need >> 20, events_in=ev)
    assert (woken["events_out"] > ev).all()


def test_a_clock_of_zeros_fires_4096_events_per_step():
    N, Q, n, S = 3, 3, 5, 2
    s = q3.random_placements(N, n, 12, Q=Q)
    seeds = abi.seeds_for(31, n)
    tabs = _tables([0.0] * S)  # every weight 2^24: W > 0 whatever the placement is
    zero = (0, np.zeros(256, dtype=np.uint32))
    got = nfold.nfold_queens_host(N, s, seeds, tabs, 1, Q=Q, clock=zero, hist=True)
    assert (got["events_out"] == S << abi.NFOLD_TIME_BITS).all() and (got["need_out"] == 0).all()
    assert (got["best_step"] <= S).all() and (got["weight_out"] == Q * (N ** 3 - Q) << 24).all()
    n3.assert_equal({k: v[:1] for k, v in got.items()}, n3.nfold_many(N, s[:1], seeds[:1], tabs, 1, zero, Q=Q), "a clock of zeros")


def test_a_repeated_placement_is_flagged_and_handed_back_unmoved():
    N, Q, n = 5, 25, 6
    s = q3.random_placements(N, n, 9, Q=Q, over=True)
    s[1, 3:6] = s[1, 0:3]  # queens 0 and 1 in one cell
    s[4] = 200  # every queen clamped into the last cell
    seeds = abi.seeds_for(3, n)
    need = np.arange(1, n + 1, dtype=np.uint64) << 40
    ev = np.arange(n, dtype=np.int64) * 7 + (1 << 35)
    for kw in (dict(), dict(need_in=need, events_in=ev)):
        got = nfold.nfold_queens_host(N, s, seeds, _tables(), 20, Q=Q, hist=True, **kw)
        n3.assert_equal(got, n3.nfold_many(N, s, seeds, _tables(), 20, nfold.clock_tables("exp"), Q=Q, **kw), f"repeated placements {sorted(kw)}")
        assert [int(f) for f in got["flags"]] == [0, 1, 0, 0, 1, 0] and abi.NFOLD3D_REPEATED == 1
        for r in (1, 4):
            e = q3.pairwise_energy(N, s[r])
            assert got["energy_in"][r] == got["energy_out"][r] == got["best_energy"][r] == e and (got["energy_hist"][r] == e).all()
            assert (got["state"][r] == np.minimum(s[r], N - 1)).all() and (got["best_state"][r] == got["state"][r]).all()
            assert got["weight_out"][r] == 0 and got["best_step"][r] == 0 and got["n_uphill"][r] == 0 and got["n_flat"][r] == 0
            assert got["events_out"][r] == (ev[r] if kw else 0)
            # need_out is need_in, or without one the need drawn from block events_in
            M = Q * (N ** 3 - Q)
            assert int(got["need_out"][r]) == (int(need[r]) if kw else M * n3.ell(n3.block(int(seeds[r]), 0)[2], *nfold.clock_tables("exp")))
        assert got["energy_out"][4] == Q * (Q - 1) // 2


def test_wide_arithmetic_a_need_beyond_2_to_the_52_against_python_integers():
    s, seeds, need, rows, got = n3.wide_need_case(nfold, abi)
    left = 1 << 43
    W = [int(w) for w in got["weight_out"]]
    print("W under [1, 0]:", W, "need_in:", [int(v) for v in need], "need_out:", [int(v) for v in got["need_out"]])
    for r in range(3):  # nothing fires: the state and W stay, and need falls by the 96-bit product's quotient
        assert int(need[r]) << 12 >= 1 << 64 and int(need[r]) // W[r] >= 1 << 32 and left * W[r] >= 1 << 64
        assert got["events_out"][r] == 0 and (got["state"][r] == s[r]).all()
        assert int(got["need_out"][r]) == int(need[r]) - ((left * W[r]) >> 12)
    # chain 3 fires once, 5 units before the end, from both quotients; its next need, M 2^24, does not fire within them.  (The clock
    # alone, in Python integers: the restatement's matrices of 1 024 queens by 32 768 cells are not built here.)
    W0 = int(nfold.nfold_queens_host(32, s[3:], seeds[3:], rows, 1, clock="mean", need_in=np.array([1 << 57], dtype=np.uint64))["weight_out"][0])
    M = 1024 * (32 ** 3 - 1024)
    assert int(need[3]) << 12 >= 1 << 64 and int(need[3]) // W0 < 1 << 32 and (int(need[3]) << 12) // W0 == left - 5
    assert got["events_out"][3] == 1 and got["best_step"][3] in (0, (1 << 31) - 1) and len(n3.moves(32, s[3:], got["state"][3:])[0]) == 1
    assert ((M << 24) << 12) // W[3] > 5 and int(got["need_out"][3]) == (M << 24) - ((5 * W[3]) >> 12)
    assert got["energy_out"][3] <= got["energy_in"][3]  # the row [1, 0] lets nothing rise


def test_wide_arithmetic_the_largest_m_at_beta_zero_against_python_integers():
    """N = 32 at the largest Q the LDS admits, beta = 0, the mean clock, one step: W = M 2^24 = need, tau = 2^12 = left, and the one
    event is pair number floor(U / 2^24) in the order q ascending, free cells ascending, U from the whole 128-bit product."""
    N = 32
    Q = n3.largest_queens(abi, N)
    C = N ** 3
    M = Q * (C - Q)
    s = q3.random_placements(N, 1, 5, Q=Q)
    seeds = abi.seeds_for(4294967000, 1)
    got = nfold.nfold_queens_host(N, s, seeds, _tables([0.0]), 1, Q=Q, clock="mean", hist=True)
    assert got["events_out"][0] == 1 and int(got["weight_out"][0]) == M << 24 and got["best_step"][0] in (0, 1)
    x = n3.block(int(seeds[0]), 0)
    U = (((x[0] << 32) | x[1]) * (M << 24)) >> 64
    assert (M << 24) * ((1 << 64) - 1) >= 1 << 115  # the product is wider than 64 + 51 bits
    q, k = divmod(U >> 24, C - Q)
    z = q3.clamp(N, s[0])
    free = np.setdiff1d(np.arange(C), n3.index_of(N, z))
    t = int(free[k])
    mq, mt = n3.moves(N, s, got["state"])
    assert [int(v) for v in mq] == [q] and [int(v) for v in mt] == [t]
    assert int(got["need_out"][0]) == M * n3.ell(n3.block(int(seeds[0]), 1)[2], *nfold.clock_tables("mean")) == M << 24  # left = 0: nothing was spent
    recount = nfold.nfold_queens_host(N, got["state"], seeds, nfold.weight_tables([]), 1, Q=Q)
    assert got["energy_out"][0] == recount["energy_in"][0] and recount["flags"][0] == 0


def _wilson_hilferty(df, z=3.090232306167813):  # the 99.9 % quantile of chi^2 with df degrees of freedom
    return df * (1 - 2 / (9 * df) + z * np.sqrt(2 / (9 * df))) ** 3


@pytest.mark.parametrize("clock", nfold.CLOCKS)
@pytest.mark.parametrize("beta", (0.5, 1.0, 2.0))
@pytest.mark.parametrize("Q", (3, 4))
def test_stationary_distribution_is_boltzmann(Q, beta, clock):
    """N = 3 with Q = 3 and Q = 4: the histogram of energy_out of 8 192 chains from random placements after one segment of 300
    Metropolis steps at constant beta against the exact Boltzmann weights of all ordered placements of Q queens on distinct cells
    (tests/heatbath3d_util.py), for three seed bases and both clocks.  Bins of expected count < 5 are merged; chi^2 must stay below its
    99.9 % quantile.  Seeded, hence deterministic: a failure is a finding about the rule or its implementation.
    Measured with the Philox stream, chi^2 (degrees of freedom; bound), seed bases 42, 100000, 4000000000:
      Q = 3, beta 0.5 (3; 16.27): exp 6.41, 0.26, 3.84; mean 1.76, 0.22, 1.71
      Q = 3, beta 1.0 (3; 16.27): exp 8.22, 7.24, 1.15; mean 6.05, 4.80, 2.81
      Q = 3, beta 2.0 (3; 16.27): exp 2.88, 1.46, 1.21; mean 5.05, 0.51, 2.85
      Q = 4, beta 0.5 (6; 22.46): exp 5.95, 7.72, 5.24; mean 5.84, 6.41, 7.33
      Q = 4, beta 1.0 (6; 22.46): exp 8.25, 3.17, 7.37; mean 5.92, 3.24, 4.03
      Q = 4, beta 2.0 (5; 20.52): exp 5.43, 6.53, 3.05; mean 4.38, 1.98, 14.79"""
    N, n, steps = 3, 8192, 300
    count, exact = h3.boltzmann_energy_shares(N, Q, beta)
    assert count == int(np.prod(np.arange(N ** 3, N ** 3 - Q, -1))) and abs(sum(exact.values()) - 1) < 1e-12
    try:
        from scipy.stats import chi2

        quantile = lambda df: float(chi2.ppf(0.999, df))  # noqa: E731
    except ImportError:
        quantile = _wilson_hilferty
    tabs = _tables([beta])
    for base in (42, 100000, 4000000000):
        s = q3.random_placements(N, n, base % 1000, Q=Q)
        got = nfold.nfold_queens_host(N, s, abi.seeds_for(base, n), tabs, steps, Q=Q, clock=clock)
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
        print(f"Q={Q} beta={beta} {clock} seeds {base}+: chi^2 = {chi:.2f} with {df} degrees of freedom, bound {quantile(df):.2f}")
        assert chi < quantile(df), f"Q={Q}, beta={beta}, {clock}, seeds {base}+: chi^2 = {chi:.2f} >= {quantile(df):.2f} ({df} degrees of freedom)"
