"""CPU only: the crafted near-tie cases of the Philox stream (near_tie_util.PHILOX_CASES, exchange_tie_util.PHILOX_CASES).

With MCQ_RNG_PHILOX4X32_10 the stream_words output is 0 by contract, so the crafting reads the number of words a chain drew from a side
channel of the oracle (oracle.run(words=True)).  Here that count is held three ways -- against stream_words on the MT19937 stream, against
a locator that uses no count at all on the Philox stream (near_tie_util.locate_by_bisection), and against the oracle's swap decision under
exchange -- the cases are held to the rows of SWEEP_TABLE they are there for, the oracle (naive and fast) to the crafted counts and to each
decision recomputed in Python, and the MT19937 crafting to what it gave before the generator became a parameter of a case."""
import hashlib
import math

import numpy as np
import pytest

import mcq_amd
from oracle import oracle
from tests import exchange_tie_util as xt
from tests import near_tie_util as nt
from tests import test_exchange_ties_host as host_x
from tests import test_near_ties_host as host
from tests import variant_cases as vc

abi = mcq_amd.abi
PLAIN = [c.name for c in nt.PHILOX_CASES]
EXCHANGE = [c.name for c in xt.PHILOX_CASES]
F = abi.SWEEP_VARIANT_FIELDS


def _row(case):
    v = mcq_amd._lib.sweep_variant(case.params(case.base_table()))
    return tuple(int(v[k]) for k in F)


def test_the_cases_run_every_philox_row_of_the_table():
    """26 plain rows and 7 under exchange, each selected by exactly the case that names it; remove a case and a row is missing."""
    plain = {c.name: _row(c) for c in nt.PHILOX_CASES}
    exch = {c.name: _row(c) for c in xt.PHILOX_CASES}
    for name, row in {**plain, **exch}.items():
        v = dict(zip(F, row))
        assert v["PHILOX"] == 1 and v["EXCH"] == (name in exch) and not (v["CAND5"] or v["EARLYU"] or v["SLIM"] or v["CNT"] or v["WIDE"]), (name, v)
    short = {name: tuple(dict(zip(F, row))[k] for k in ("MODE", "G", "PATIENCE", "NT", "REDUCED", "NC")) for name, row in plain.items()}
    short_x = {name: tuple(dict(zip(F, row))[k] for k in ("MODE", "G", "NT", "NC")) for name, row in exch.items()}
    assert short == nt.PHILOX_ROW and short_x == xt.PHILOX_ROW
    assert all(not (dict(zip(F, row))["PATIENCE"] or dict(zip(F, row))["REDUCED"]) for row in exch.values())
    assert len(set(short.values())) == len(short) == 26 and set(short.values()) == nt.PHILOX_ROWS
    assert len(set(short_x.values())) == len(short_x) == 7 and set(short_x.values()) == xt.PHILOX_EXCHANGE_ROWS
    # ... and these are all the PHILOX rows there are: of the case table of tests/variant_cases.py and of SWEEP_TABLE itself
    for table in ({r for r, _ in vc.CASES}, set(vc.reachable_rows())):
        philox = {r for r in table if r[F.index("PHILOX")]}
        assert len(philox) == 33 and philox == set(plain.values()) | set(exch.values()), sorted(philox ^ (set(plain.values()) | set(exch.values())))
    for c in nt.PHILOX_CASES + xt.PHILOX_CASES:  # the shapes: sets of 16 chains (32 at 2 lanes), a launch of 128 chains x 470 steps at the most
        assert c.rng == "philox" and c.n_sets == 4 and c.n_chains <= 128 and 300 <= c.n_steps <= 470 and c.lanes in (2, 4, 8, 16)
    assert {c.R for c in xt.PHILOX_CASES} == {2, 4, 8, 16}
    seeds = [c.seed for c in nt.CASES + xt.CASES + nt.PHILOX_CASES + xt.PHILOX_CASES]
    assert len(set(seeds)) == len(seeds), "every case its own seed"


@pytest.mark.parametrize("name", PLAIN)
def test_oracle_counts_the_crafted_philox_ties_and_decides_as_recomputed(name):
    """The plan of the case is met, and the oracle, naive and fast, counts the crafted ties and decides each crafted step as
    u < math.exp(-beta dE) does; its stream_words stays 0."""
    case = nt.CASES_BY_NAME[name]
    table, points = nt.crafted(name)
    nt.check_plan_was_met(case, points)
    if case.patience is not None:  # the reduced plan plus one point behind a stop
        assert nt.kinds(points)["behind"] >= 1 and nt.kinds(points)["count"] >= 16
    host.oracle_counts_the_crafted_ties_and_decides_as_recomputed(name)
    res = oracle.run(case.params(table, trace=True), case.seeds(), n_threads=4, words=True)
    assert not res["stream_words"].any() and (res["rng_words"] > 2 * res["steps_executed"].astype(np.uint64)).all()


@pytest.mark.parametrize("name", EXCHANGE)
def test_oracle_counts_the_crafted_philox_ties_and_swaps_as_recomputed(name):
    case = xt.CASES_BY_NAME[name]
    table, points = xt.crafted(name)
    xt.check_plan_was_met(case, points)
    host_x.oracle_counts_the_crafted_ties_and_swaps_as_recomputed(name)
    res = oracle.run(case.params(table), case.seeds(), n_threads=4, fast=True, words=True)
    assert not res["stream_words"].any() and (res["rng_words"] > 2 * case.n_steps).all()


# ---- the word count ------------------------------------------------------------------------------------------------------------------

def test_word_count_is_stream_words_on_the_mt19937_stream():
    """Every MT19937 near-tie case, plain and under exchange, under its crafted table: the side channel equals the output of the contract."""
    case = nt.CASES[0]
    assert "rng_words" not in oracle.run(case.params(case.base_table()), case.seeds(), trace=False, states=False, fast=True), "only on request"
    for mod in (nt, xt):
        for case in mod.CASES:
            table, _ = mod.crafted(case.name)
            for fast in (True,) if case.N > 17 else (False, True):
                res = oracle.run(case.params(table), case.seeds(), trace=case.trace, states=False, n_threads=4, fast=fast, words=True)
                assert res["rng_words"].dtype == np.uint64 and (res["rng_words"] > 0).all()
                np.testing.assert_array_equal(res["rng_words"] & np.uint64(0xFFFFFFFF), res["stream_words"].astype(np.uint64), err_msg=f"{case.name} fast={fast}")


# (case, index of the crafted point): board and full_3d, the first point of a run and later ones, ties and bracket points
LOCATED = (("p_board6_g2", 0), ("p_board6_g2", 40), ("p_board12_g4", 1), ("p_board17_g16", 3), ("p_full3d6_g4", 0), ("p_full3d6_g4", 30),
           ("p_full3d12_g8", 2), ("p_full3d17_g16", 1))


@pytest.mark.parametrize("name,index", LOCATED)
def test_word_count_names_the_pair_the_bisection_finds(name, index):
    """The pair of words that the count names as the uniform of a crafted step is the one a locator finds that never sees a count: it
    bisects beta(s) on the oracle's accept bit of step s and looks the bracketed u up in the Philox stream."""
    case = nt.CASES_BY_NAME[name]
    table, points = nt.crafted(name)
    pt = points[index]
    assert pt["kind"] != "behind" and pt["dE"] > 0
    words, u, pairs = nt.locate_by_bisection(case, table, pt["chain"], pt["step"])
    assert pairs == 1, f"{name}: {pairs} word pairs of the stream inside the bisection's bracket"
    p = abi.make_params(case.N, pt["step"] + 1, "random", case.base_schedules()[0], 1, mcmc_type=case.mode, rng="philox")
    tab = np.ascontiguousarray(table[pt["set"]: pt["set"] + 1, : pt["step"] + 1])
    p._schedules, p.beta_table = None, tab.ctypes.data
    seed = int(case.seeds()[pt["chain"]])
    for fast in (False, True):
        res = oracle.run(p, np.array([seed], dtype=np.uint32), states=False, fast=fast, words=True)
        assert int(res["rng_words"][0]) == words < nt.LOCATOR_WORDS and int(res["stream_words"][0]) == 0, (name, pt["chain"], pt["step"], fast)
    assert u == pt["u"]
    w = oracle.rng_stream(seed, "u32", words, rng="philox")
    assert nt.uniform_of(w[-2], w[-1]) == u


def test_word_count_locates_the_uniform_of_a_philox_swap():
    """Under exchange the uniform of an event is the last pair of the lower chain's words after the event's step.  Located through the
    count alone, it reproduces the oracle's swap decision -- recomputed in Python, in the oracle's order -- at tie points, where a
    neighbouring pair of the stream would decide by chance."""
    checked = {True: 0, False: 0}
    for name in ("px_board12_g8", "px_full3d6_g4"):
        case = xt.CASES_BY_NAME[name]
        table, points = xt.crafted(name)
        for pt in xt.swap_points(points):
            if pt["kind"] != "count":
                continue
            t, s = pt["set"], pt["step"]
            sub, lo = case.one_set(t), t * case.set_chains
            a = pt["chain"] - lo
            before, after = (oracle.run(sub.params(table[t: t + 1, :n], n_steps=n), sub.seeds(), states=False, words=True) for n in (s, s + 1))
            w = oracle.rng_stream(int(sub.seeds()[a]), "u32", int(after["rng_words"][a]), rng="philox")
            u = nt.uniform_of(w[-2], w[-1])
            dEab = int(after["final_energy"][a]) - int(after["final_energy"][pt["partner"] - lo])
            swap = u < math.exp(xt.swap_x(float(table[t, s]), float(case.ladder[pt["t"]]), float(case.ladder[pt["t"] + 1]), dEab))
            assert int(before["exchange_rung"][a]) == pt["t"] and (int(after["exchange_rung"][a]) == pt["t"] + 1) == swap, (name, pt)
            assert u == pt["u"] and swap == pt["swap"] and abs(pt["ulps"]) in (2, 3)
            for shift in (2, 4):  # the pairs in front of it are other numbers altogether: a count off by a draw would not pass
                assert nt.uniform_of(w[-2 - shift], w[-1 - shift]) != u
            checked[swap] += 1
    assert checked[True] >= 2 and checked[False] >= 2, checked


# ---- the MT19937 crafting is what it was ---------------------------------------------------------------------------------------------

def _digest(table, points):
    h = hashlib.sha256(np.ascontiguousarray(table).tobytes())
    for pt in points:
        h.update(repr(sorted((k, (float(v).hex() if isinstance(v, float) else v)) for k, v in pt.items())).encode())
    return h.hexdigest()


# name: (SHA-256 over the table's bytes and every field of every point, points, then chain, step, u and beta of the first point), computed
# with the crafting as it stood before a case carried its generator
BEFORE = {
    "board12_g4": ("dfbe0d154c7aee11f2793d7f31f77287341c9d49abfc50be1bfc56534aa90b3f", 108, 0, 6, "0x1.be0377b5b65f2p-2", "0x1.7a40c9a46c920p-4"),
    "board12_patience": ("dbf01b3879b3cb4cf2e189c35db3bec4802e3c7ca27b2df9bcd208b6bd73ce80", 55, 0, 13, "0x1.86e330e08a0f1p-1", "0x1.1461f4a178109p-3"),
    "x_full3d6_g4": ("efbe45d946a65d09d60491c0b5d7960bfe2cec25cbee9abe8833aac25436b5dd", 76, 0, 3, "0x1.acdf867a38543p-1", "0x1.2e5be42bc56fep-6"),
    "x_board12_g8": ("04cd21b311a55e3219d73229d5c4904279c242c60d2ad94b93cf8d744b616ac1", 76, 13, 3, "0x1.df41baa7912b2p-1", "0x1.437d188a261e5p-4"),
}


@pytest.mark.parametrize("name", sorted(BEFORE))
def test_mt19937_crafting_is_unchanged(name):
    mod = xt if name.startswith("x_") else nt
    assert mod.CASES_BY_NAME[name].rng == "mt19937"
    table, points = mod.crafted(name)
    sha, n, chain, step, u, beta = BEFORE[name]
    first = points[0]
    assert (len(points), first["chain"], first["step"], first["u"].hex(), first["beta"].hex()) == (n, chain, step, u, beta)
    assert _digest(table, points) == sha
