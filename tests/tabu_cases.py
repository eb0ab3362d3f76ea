"""The inputs that tests/test_tabu.py (GPU) and tests/test_tabu_host.py (CPU) share, and their references, each computed once and never
changed: the comparisons at both ends of every instantiation of the kernel with the restatement of whole runs, the sleeping runs that
wake across the move of the stamp base, the boards at the ends of the packed key, and the runs across first_iter = 2^32."""
import functools

import numpy as np

import mcq_amd
from tests import quench_util as qu
from tests import tabu_util as tu

abi = mcq_amd.abi
quench = mcq_amd.quench

# the instantiations are padded N = 4, 8, 12, 16, 24, 32: both ends of each
GROUPS = {4: (2, 4), 8: (5, 8), 12: (9, 12), 16: (13, 16), 24: (17, 24), 32: (25, 32)}
DEEP_FROM = 17     # from this N on the comparisons start deep in a walk: a short run from a random board only descends
DEEP_ITERS = 2500
DEEP_TENURE = dict(tenure=8, tenure_rand=4, tenure_conf=2)
ALL = dict(hist=True, tabu_out=True)


def iters(N):
    return 300 if N < DEEP_FROM else 200


def stamps(N, n, seed, hold):
    """Random stamps of up to 40 iterations; chain 0 has every entry tabu for `hold` iterations."""
    tin = np.random.RandomState(seed).randint(0, 41, size=(n, N ** 3)).astype(np.uint16)
    tin[0] = hold
    return tin


@functools.lru_cache(maxsize=None)
def _deep(N):
    """3 boards of N >= DEEP_FROM behind DEEP_ITERS iterations of the host code, with their stamps and best energies: inputs only."""
    s = qu.random_boards(N, 3, 100 * N, over=True)
    return quench.tabu_host(N, s, abi.seeds_for(900 + N, 3), DEEP_ITERS, tabu_out=True, **DEEP_TENURE)


@functools.lru_cache(maxsize=None)
def cases(N):
    """(boards, seeds, keywords) of the comparisons at N: every chain count; tenure = 8192 at N <= 3 and a start with every entry of a
    chain tabu under a floor of 0 are the stalls, random stamps the aspiration; at N >= DEEP_FROM the walk goes on from _deep."""
    if N >= DEEP_FROM:
        d = _deep(N)
        deep = dict(first_iter=DEEP_ITERS, tabu_in=d["tabu_out"], best_floor=d["best_energy"], **DEEP_TENURE)
        s = qu.random_boards(N, 3, 100 * N + 3, over=True)
        floor = np.full(3, 1 << 30, dtype=np.int32)
        floor[0] = 0
        return ((d["state"][:1], abi.seeds_for(900 + N, 1), {k: (v[:1] if isinstance(v, np.ndarray) else v) for k, v in deep.items()}),
                (d["state"], abi.seeds_for(900 + N, 3), deep),
                (s, abi.seeds_for(500 + N, 3), dict(tenure=3, tenure_rand=5, tabu_in=stamps(N, 3, N, 50), best_floor=floor)))
    floor = np.full(5, 1 << 30, dtype=np.int32)
    floor[0] = 0
    return ((qu.random_boards(N, 1, 100 * N + 1, over=True), abi.seeds_for(500 + N, 1), dict(tenure=8192 if N <= 3 else N // 2 + 1, tenure_rand=3)),
            (qu.random_boards(N, 5, 100 * N + 5, over=True), abi.seeds_for(510 + N, 5), dict(tenure=2, tenure_rand=5, tenure_conf=8, tabu_in=stamps(N, 5, N, 100),
                                                                                               best_floor=floor)),
            (qu.random_boards(N, 65, 100 * N + 65, over=True), abi.seeds_for(520 + N, 65), dict(tenure=N, tenure_rand=N, tenure_conf=4)))


@functools.lru_cache(maxsize=None)
def restated(N, i, r):
    """Chain r of case i at N through the restatement, the whole run of iters(N) iterations."""
    s, seeds, kw = cases(N)[i]
    one = {k: (v[r] if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    return tu.tabu(N, s[r], int(seeds[r]), iters(N), **one)


def row(res, r):
    """Chain r of a result of many chains, in the form of tu.tabu's."""
    return {k: np.asarray(res[k])[r] for k in tu.FIELDS}


# The sleeping runs (tests/tabu_util.py) at both ends of the four large instantiations.  The chains are as many as keep a GPU test at a
# few seconds: an iteration of the kernel takes 26 us at N = 32 whatever the chains, one of the restatement 5 ms per chain
SLEEP_CHAINS = {9: 3, 12: 2, 13: 3, 16: 2, 17: 3, 24: 1, 25: 2, 32: 1}
SLEEP_ITERS = tu.REBASE + 332
VARIANTS = ("spread", "edge")
# (N, variant) -> the seed of tabu_in where the default, 1000 + N, leaves a group of tests/test_tabu_host.py without one of the three
# confusions of the stamps next to the mark
SLEEP_SEED = {(13, "edge"): 31013, (25, "edge"): 11025}


# chains that only tests/test_tabu_host.py adds behind those, so that every N has two or three there
SLEEP_MORE = {24: 1, 25: 1, 32: 1}


def sleep_inputs(N, variant, more=False):
    """(boards, seeds, tabu_in, W) of the sleeping runs at N; more=True: with the chains of SLEEP_MORE behind them."""
    n = SLEEP_CHAINS[N]
    tin, W = tu.sleeping(N, n, SLEEP_SEED.get((N, variant), 1000 + N), variant)
    s, seeds = qu.random_boards(N, n, 300 + N, over=True), abi.seeds_for(700 + N, n)
    if more and N in SLEEP_MORE:
        m = SLEEP_MORE[N]
        s, seeds = np.concatenate([s, qu.random_boards(N, m, 350 + N, over=True)]), np.concatenate([seeds, abi.seeds_for(750 + N, m)])
        tin = np.concatenate([tin, tu.sleeping(N, m, 5000 + N, variant)[0]])
    return s, seeds, tin, W


@functools.lru_cache(maxsize=None)
def _woken(N, variant, n_iters, r):
    s, seeds, tin, W = sleep_inputs(N, variant, True)
    return tu.wake(N, s[r : r + 1], seeds[r : r + 1], n_iters, tin[r : r + 1], W, **tu.LONGEST)


def sleep_case(N, variant, n_iters=SLEEP_ITERS, more=False):
    """(boards, seeds, tabu_in, W, the whole call's outputs restated over its window) of a sleeping run under the longest tenure; every
    chain is restated once."""
    s, seeds, tin, W = sleep_inputs(N, variant, more)
    rows = [_woken(N, variant, n_iters, r) for r in range(len(s))]
    want = {k: np.concatenate([np.asarray(x[k]) for x in rows]) for k in tu.FIELDS}
    want["trace"] = [x["trace"][0] for x in rows]
    return s, seeds, tin, W, want


def sleep_kw(N, variant, more=False):
    s, seeds, tin, _ = sleep_inputs(N, variant, more)
    return dict(tabu_in=tin, best_floor=np.zeros(len(s), dtype=np.int32), **tu.LONGEST)


def check_wakes(N, variant):
    """The coverage of a sleeping run, from the restated window: moves on both sides of the base's move, and a stamp written before it
    that keeps a candidate out after it."""
    n = tu.wake_cover(sleep_case(N, variant)[4]["trace"])
    assert n["moves_before"] >= 1 and n["moves_after"] >= 100 and n["held_across"] >= 1, f"N={N} {variant}: {n}"
    return n


# The top of the stamp range: tabu_in at the contract's ends among the sleeping stamps, most columns conflicting, the longest tenure
TOP_ITERS = tu.REBASE + 332
TOP_VALUES = (65535, 65534, 32769, 32768, 32767)


def top_inputs(N):
    """(board, seeds, tabu_in, W): one sleeping chain ("spread") from a random board whose stamps hold, at random entries, 65535, 65534,
    32769, 32768 and 32767, and 1 and 0 at entries (c, h(c)): those name no candidate while the chain sleeps, and the first move of the
    column overwrites them, so they must be loaded and must change nothing."""
    s = qu.random_boards(N, 1, 400 + N, over=True)
    tin, W = tu.sleeping(N, 1, 2000 + N, "spread")
    rs = np.random.RandomState(N)
    own = np.arange(N * N) * N + qu.clamp(N, s[0])
    at = rs.choice(np.setdiff1d(np.arange(N ** 3), own), size=20 * len(TOP_VALUES), replace=False)
    tin[0, at] = np.repeat(TOP_VALUES, 20).astype(np.uint16)
    tin[0, own] = rs.randint(0, 2, size=N * N).astype(np.uint16)
    return s, abi.seeds_for(800 + N, 1), tin, W


@functools.lru_cache(maxsize=None)
def top_case(N):
    s, seeds, tin, W = top_inputs(N)
    return s, seeds, tin, W, tu.wake(N, s, seeds, TOP_ITERS, tin, W, **tu.LONGEST)


def top_stamp(N):
    """The largest base-relative stamp that the restated window writes before the base moves, and the bound it must reach: 1024 below
    the bound below which the contract keeps them at this N, 2^15 + 8192 + 4095 + 64 N^2 / 16 + 1 (at N = 32 that is 2^15 + 2^14)."""
    top = max(tr["g"] + 1 + tr["L"] for tr in top_case(N)[4]["trace"][0] if tr["moved"] and tr["g"] < tu.REBASE)
    return top, tu.REBASE + 8192 + 4095 + 64 * N * N // 16 + 1 - 1024


# The ends of the packed key
KEY_N = (12, 16, 24, 32)
KEY_ITERS = {"flat": 30, "uphill": 80}


@functools.lru_cache(maxsize=None)
def key_case(N, kind):
    """(board, seeds, keywords, the restatement) of the flat board (30 iterations, tenure 3 + (0 .. 2)) and of the forced rise (the
    move, 49 iterations in which the stamps of 50 hold all but the centre queen, then 30 iterations of descent)."""
    seeds = abi.seeds_for(600 + N, 1)
    if kind == "flat":
        b, kw = tu.flat_board(N), dict(tenure=3, tenure_rand=2)
    else:
        b, tin = tu.uphill_board(N)
        kw = dict(tenure=3, tenure_rand=2, tabu_in=tin, best_floor=np.zeros(1, dtype=np.int32))
    return b, seeds, kw, tu.tabu_many(N, b, seeds, KEY_ITERS[kind], **kw)


def check_key(N, kind):
    """The coverage of a key case, from the restatement: a delta within 2 of -max a(c, k) on the flat board, within 4 of +max a(c, k) on
    the other, and ties among the candidates of such a move (rho decides at a large |delta|)."""
    b, _, _, want = key_case(N, kind)
    a_max = int(tu.table(N, qu.clamp(N, b[0])).max())
    moves = [tr for tr in want["trace"][0] if tr["moved"]]
    if kind == "flat":
        big = [tr for tr in moves if tr["delta"] <= -(a_max - 2)]
    else:
        big = [tr for tr in moves if tr["delta"] >= a_max - 4]
        # the first iteration is the rise; while the stamps of 50 hold, the centre queen alone goes back and forth as its own short stamps expire
        assert moves[0] is want["trace"][0][0] and big[:1] == moves[:1] and sum(not tr["moved"] for tr in want["trace"][0][1:50]) >= 30
    assert big and a_max >= 3 * (N - 1), f"N={N} {kind}: a_max {a_max}, deltas {[tr['delta'] for tr in moves]}"
    assert any(tr["ties"] > 1 and abs(tr["delta"]) >= a_max // 2 for tr in moves), f"N={N} {kind}: no tie at a large |delta|"
    return a_max, [tr["delta"] for tr in big]


# first_iter on both sides of 2^32
WORD_CASES = ((4, 3, (1 << 32) - 30), (6, 2, (1 << 32) - 1), (13, 2, 1 << 32), (25, 1, (1 << 33) - 20))
WORD_ITERS = 60
WORD_TENURE = dict(tenure=3, tenure_rand=5, tenure_conf=4)


@functools.lru_cache(maxsize=None)
def word_case(N, n, first):
    s, seeds = qu.random_boards(N, n, 70 + N, over=True), abi.seeds_for(11 + N, n)
    return s, seeds, tu.tabu_many(N, s, seeds, WORD_ITERS, first_iter=first, **WORD_TENURE)


def low_word_hist(fn, N, s, seeds, first, **extra):
    """The histories that a counter without its high word gives for the run from `first`: iteration g draws as g mod 2^32 does, so the
    run is the one from first mod 2^32 up to 2^32 and then, the stamps carried, the one from 0.  fn: tu.tabu_many, tabu_host, tabu_states."""
    lo = first & 0xFFFFFFFF
    a = min(WORD_ITERS, (1 << 32) - lo)
    p = fn(N, s, seeds, a, first_iter=lo, **WORD_TENURE, **extra)
    if a == WORD_ITERS:
        return np.asarray(p["energy_hist"])
    q = fn(N, p["state"], seeds, WORD_ITERS - a, first_iter=0, tabu_in=p["tabu_out"], best_floor=p["best_energy"], **WORD_TENURE, **extra)
    return np.concatenate([p["energy_hist"], np.asarray(q["energy_hist"])[:, 1:]], axis=1)
