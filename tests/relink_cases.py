"""The inputs that tests/test_relink_host.py puts to mcq_relink_host and its restatement, and tests/test_relink.py to the kernel: per N a
list of calls -- minima of random boards relinked with their neighbour, random boards with bytes >= N, the guide equal to the placement
(d0 = 0) and a height off in every column (d0 = N^2), and the window of candidates at its edges --, each computed once and shared."""
import functools

import numpy as np

import mcq_amd
from tests import quench_util as qu
from tests import relink_util as ru

FULL = (2, 3, 4, 5, 8, 9, 12)          # every chain against the restatement
CHAIN0 = (13, 16, 17, 24, 25, 32)      # chain 0 against the restatement
ALL_N = FULL + CHAIN0
SEARCHES = ("single", "pairs")
SHORT = 40  # the steps of the cut walk between random boards and, beyond N = 16, of the two walks whose window holds one candidate and none


def group(N):
    """The instantiation of the kernel that runs N."""
    return next(p for p in (4, 8, 12, 16, 24, 32) if N <= p)


def chains(N):
    return 6 if N <= 5 else 4 if N <= 12 else 2


def edge_dist(N):
    """min_dist of the two calls whose window holds one candidate and none: a quarter of the columns up to N = 16, SHORT / 2 beyond."""
    return max(1, N * N // 4) if N <= 16 else SHORT // 2


def cheap(N, name, kw):
    """Whether tests/test_relink.py compares chain 0 of a call with the restatement itself: beyond N = 16 the walks of at most SHORT steps,
    which the restatement runs within a second, and at N = 32 the walk of d0 = N^2 = 1 024 steps, which takes it seconds: the longest walk and
    every value of rho.  (tests/test_relink_host.py holds the host code to the restatement on chain 0 of EVERY call at every N.)"""
    return N <= 16 or bool(kw.get("max_steps")) or name in ("one candidate", "no candidate", "the guide is the placement") or (
        N == 32 and name == "every column differs")


def shifted(N, states):
    """Every column one height off, cyclically: d0 = N^2."""
    return ((np.minimum(states, N - 1).astype(np.int64) + 1) % N).astype(np.uint8)


def apart(N, states, d):
    """Guides that differ from the (clamped) states in the first d columns and nowhere else."""
    g = np.minimum(states, N - 1).astype(np.uint8)
    g[:, :d] = shifted(N, g[:, :d])
    return g


@functools.lru_cache(maxsize=None)
def cases(N):
    """[(name, states, guides, seeds, keywords, restated)]: `restated` says whether the restatement runs the case; it runs every one."""
    n, Q = chains(N), N * N
    seeds = mcq_amd.abi.seeds_for(70 + N, n)
    m = ru.minima(N, n, 11 + N)
    quarter = max(1, Q // 4)
    edge = edge_dist(N)
    # minima of the pair-move quench too (inputs only): with no candidate P* is the input, and neither local search moves on it
    pm = mcq_amd.quench.quench_pairs_host(N, m, conflicts=False)["state"]
    rnd_a, rnd_g = qu.random_boards(N, n, 21 + N, over=True), qu.random_boards(N, n, 31 + N, over=True)
    assert int(rnd_a.max()) >= N and int(rnd_g.max()) >= N
    out = [("minima", m, ru.neighbours(m), seeds, dict(min_dist=1), True),
           ("minima, a quarter", m, ru.neighbours(m), seeds, dict(min_dist=quarter), True),
           ("minima, the guide a candidate", m, ru.neighbours(m), seeds, dict(min_dist=0), True),
           ("random, bytes >= N", rnd_a, rnd_g, seeds, dict(min_dist=1), True),
           ("the guide is the placement", rnd_a, rnd_a.copy(), seeds, dict(min_dist=1), True),
           ("every column differs", m, shifted(N, m), seeds, dict(min_dist=quarter), True),
           ("one candidate", m, apart(N, m, 2 * edge), seeds, dict(min_dist=edge), True),
           ("no candidate", pm, apart(N, pm, 2 * edge - 1), seeds, dict(min_dist=edge), True),
           ("one step, below min_dist", rnd_a, rnd_g, seeds, dict(min_dist=2, max_steps=1), True),
           ("random, a cut walk", rnd_a, rnd_g, seeds, dict(min_dist=1, max_steps=min(SHORT, Q)), True),
           ("three steps", m, ru.neighbours(m), seeds, dict(min_dist=1, max_steps=min(3, Q)), True)]
    return out


@functools.lru_cache(maxsize=None)
def restated(N, i, search):
    """The restatement's result of case i at N under the local search `search`: every chain for N in FULL, chain 0 beyond."""
    name, s, g, seeds, kw, runs = cases(N)[i]
    assert runs
    rows = slice(None) if N in FULL else slice(0, 1)
    return ru.relink_many(N, s[rows], g[rows], seeds[rows], local_search=search, **kw)


@functools.lru_cache(maxsize=None)
def restated_chain0(N, i, search):
    """The restatement's result of chain 0 of case i alone: what the comparison of the kernel takes, at every N."""
    name, s, g, seeds, kw, runs = cases(N)[i]
    assert runs
    return ru.relink_many(N, s[:1], g[:1], seeds[:1], local_search=search, **kw)


@functools.lru_cache(maxsize=None)
def hosted(N, i, search):
    """The host code's outputs of case i, histories included."""
    name, s, g, seeds, kw, runs = cases(N)[i]
    return mcq_amd.quench.relink_host(N, s, g, seeds, local_search=search, hist=True, **kw)


@functools.lru_cache(maxsize=None)
def coverage(search, grp):
    """The coverage of one group (instantiation) under one local search: the steps' traces of the restatement (every chain for N in FULL,
    chain 0 beyond) and the outputs of the host code on every chain."""
    cov = ru.Coverage()
    for N in (n for n in ALL_N if group(n) == grp):
        for i, (name, s, g, seeds, kw, runs) in enumerate(cases(N)):
            cov.add_traces(grp, restated(N, i, search)["trace"])
            cov.add_outputs(grp, ru.host_cover(N, hosted(N, i, search), g, kw["min_dist"]))
    return cov
