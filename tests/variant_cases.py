"""The explicit case table of the sweep kernel's instantiations: for every row of SWEEP_TABLE (csrc/mcq_hip.hip) that a parameter
block can reach, the launches that select it -- at the smallest and the largest N of the row, at the smallest chain count that still
leaves a partially filled wavefront -- as literals.  No tests here: tests/test_variant_cases.py holds the table to the library's
selection and to the conditions below on the CPU, tests/test_every_variant.py runs every case on the GPU against the oracle.

A case is dict(mode, N, chains, steps, init, sched, lanes, seed) plus, where they differ from the defaults of `case()`: patience, trace,
rng, flags, Q, exch = (every, rungs, lowest, highest multiplier), inits (one init mode per schedule set).  More than one schedule in
`sched` makes schedule sets of chains / len(sched) chains each.  tools/derive_variant_cases.py derives the table (mcq_sweep_variant
needs no GPU) and rewrites the lines between the two markers; nothing is searched at import.

How the cases are chosen (the CPU test asserts what can be asserted):
* N: the smallest and the largest N that select the row, as two cases where they differ -- and N = 3 besides N = 2, where every cell
  attacks every other, no move changes the energy and none is rejected.
* chains: two full wavefronts and one chain more, 2 * (64 / G) + 1; five for the 64-bit full_3d rows; schedule sets in multiples of
  16 (32 at two lanes); exchange ladders in whole ladders.  No case has more than 256 chains but those of LARGE_ROWS, which only a
  launch beyond the "roomy" thresholds of select_sweep_variant takes: they run the smallest count that selects them.
* steps: at least 300 and no multiple of 16, so that a chain passes several MT19937 generations and ends inside a history block,
  an accept-bit word and a reduced-trace block.
* PATIENCE rows: a patience and a schedule under which some chains stop early and some run to the end (N = 2: all stop).
* EXCH rows: a ladder as wide as the lane count allows (16 rungs at most) and ladders of two, several to a wavefront.
* REDUCED rows: one case with two schedule sets of their own init modes, one with a single schedule and a ragged chain count.
* SLIM rows: a case with Q != N^2 where the row takes one (N as a compile-time constant comes with Q = N^2).
"""
import numpy as np

import mcq_amd
from tests.test_sweep_variant import KNOWN_UNREACHED, _table_rows

abi = mcq_amd.abi

LIN = {"type": "linear_annealing", "beta_start": 1.0, "beta_end": 3.0}
EXP = {"type": "exponential_annealing", "beta_start": 0.5, "beta_end": 4.0}
LOG = {"type": "logarithmic_annealing", "beta_start": 0.3, "beta_end": 2.5}
SIN = {"type": "sinusoidal_annealing", "beta_start": 0.5, "beta_end": 5.0}
CONST = {"type": "constant", "beta_const": 1.0}
WARM = {"type": "constant", "beta_const": 0.4}
COLD = {"type": "linear_annealing", "beta_start": 2.0, "beta_end": 6.0}
CNT = abi.FLAG_LINE_COUNTERS
MAX_CHAINS = 256  # of every case outside LARGE_ROWS

# The rows no small launch selects, and the smallest chain count that does (found by bisection over mcq_sweep_variant on a device of
# 1 024 SIMDs: the 8-lane kernels leave the early-probe form beyond 16 384 chains, the 16-lane ones beyond 8 192).
LARGE_ROWS = {
    (0, 8, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0): 16385,
    (0, 8, 0, 3, 1, 0, 0, 0, 0, 0, 0, 0, 0): 16385,
    (0, 8, 0, 3, 1, 0, 24, 0, 0, 0, 0, 0, 0): 16385,
    (0, 8, 1, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0): 16385,
    (0, 16, 0, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0): 8193,
}


def case(mode, N, chains, steps, init, sched, lanes, seed, patience=None, trace=True, rng="mt19937", flags=0, Q=None, exch=None, inits=None):
    return dict(mode=mode, N=N, chains=chains, steps=steps, init=init, sched=tuple(sched), lanes=lanes, seed=seed, patience=patience, trace=trace,
                rng=rng, flags=flags, Q=Q, exch=exch, inits=inits)


# (row, case): MODE, G, PATIENCE, NT, REDUCED, PHILOX, NC, EXCH, CAND5, EARLYU, SLIM, CNT, WIDE
CASES = [
    # --- table begin (tools/derive_variant_cases.py --write)
    ((0, 2, 0, 2, 0, 0, 0, 0, 1, 0, 0, 0, 0), case("board", N=2, chains=65, steps=333, init="random", sched=(LIN,), lanes=2, seed=1000)),
    ((0, 2, 0, 2, 0, 0, 0, 0, 1, 0, 0, 0, 0), case("board", N=3, chains=65, steps=389, init="latin", sched=(EXP,), lanes=2, seed=2000)),
    ((0, 2, 0, 2, 0, 0, 0, 0, 1, 0, 0, 0, 0), case("board", N=4, chains=65, steps=470, init="klarner", sched=(LOG,), lanes=2, seed=3000)),
    ((0, 2, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=6, chains=65, steps=315, init="random", sched=(SIN,), lanes=2, seed=4000)),
    ((0, 2, 0, 3, 0, 0, 0, 0, 1, 0, 0, 0, 0), case("board", N=5, chains=65, steps=333, init="latin", sched=(CONST,), lanes=2, seed=5000)),
    ((0, 2, 0, 4, 0, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=7, chains=65, steps=389, init="klarner", sched=(LIN,), lanes=2, seed=6000)),
    ((0, 2, 0, 4, 0, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=8, chains=65, steps=470, init="random", sched=(EXP,), lanes=2, seed=7000)),
    ((0, 2, 0, 5, 0, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=9, chains=65, steps=315, init="latin", sched=(LOG,), lanes=2, seed=8000)),
    ((0, 2, 0, 5, 0, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=10, chains=65, steps=333, init="klarner", sched=(SIN,), lanes=2, seed=9000)),
    ((0, 2, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=11, chains=65, steps=389, init="random", sched=(CONST,), lanes=2, seed=10000)),
    ((0, 2, 0, 6, 0, 0, 12, 0, 0, 0, 0, 0, 0), case("board", N=12, chains=65, steps=470, init="latin", sched=(LIN,), lanes=2, seed=11000)),
    ((0, 2, 0, 6, 1, 0, 12, 0, 0, 0, 0, 0, 0), case("board", N=12, chains=64, steps=315, init="klarner", sched=(EXP, LOG), lanes=2, seed=12000, trace="reduced", inits=("klarner", "random"))),
    ((0, 2, 0, 6, 1, 0, 12, 0, 0, 0, 0, 0, 0), case("board", N=12, chains=65, steps=333, init="random", sched=(LOG,), lanes=2, seed=13000, trace="reduced")),
    ((0, 2, 1, 6, 0, 0, 12, 0, 0, 0, 0, 0, 0), case("board", N=12, chains=65, steps=389, init="latin", sched=(COLD,), lanes=2, seed=14000, patience=25)),
    ((0, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=13, chains=65, steps=470, init="klarner", sched=(CONST,), lanes=2, seed=15000)),
    ((0, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=67, chains=65, steps=315, init="random", sched=(LIN,), lanes=2, seed=16000)),
    ((0, 2, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=2, chains=64, steps=333, init="latin", sched=(EXP, LOG), lanes=2, seed=17000, trace="reduced", inits=("latin", "klarner"))),
    ((0, 2, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=3, chains=65, steps=389, init="klarner", sched=(LOG,), lanes=2, seed=18000, trace="reduced")),
    ((0, 2, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=67, chains=65, steps=470, init="random", sched=(SIN,), lanes=2, seed=19000, trace="reduced")),
    ((0, 2, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=2, chains=65, steps=315, init="latin", sched=(COLD,), lanes=2, seed=20000, patience=25)),
    ((0, 2, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=3, chains=65, steps=333, init="random", sched=(LIN,), lanes=2, seed=21070, patience=200)),
    ((0, 2, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=67, chains=65, steps=389, init="random", sched=(COLD,), lanes=2, seed=22042, patience=12)),
    ((0, 2, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=2, chains=64, steps=470, init="latin", sched=(COLD, SIN), lanes=2, seed=23000, patience=25, trace="reduced", inits=("latin", "klarner"))),
    ((0, 2, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=3, chains=65, steps=315, init="random", sched=(LIN,), lanes=2, seed=24070, patience=200, trace="reduced")),
    ((0, 2, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=67, chains=65, steps=333, init="random", sched=(COLD,), lanes=2, seed=25042, patience=12, trace="reduced")),
    ((0, 4, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0), case("board", N=2, chains=33, steps=389, init="latin", sched=(LIN,), lanes=4, seed=26000)),
    ((0, 4, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0), case("board", N=3, chains=33, steps=470, init="klarner", sched=(EXP,), lanes=4, seed=27000)),
    ((0, 4, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0), case("board", N=4, chains=33, steps=315, init="random", sched=(LOG,), lanes=4, seed=28000)),
    ((0, 4, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=2, chains=32, steps=333, init="latin", sched=(SIN, CONST), lanes=4, seed=29000, trace="reduced", inits=("latin", "klarner"))),
    ((0, 4, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=3, chains=33, steps=389, init="klarner", sched=(CONST,), lanes=4, seed=30000, trace="reduced")),
    ((0, 4, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=4, chains=33, steps=470, init="random", sched=(LIN,), lanes=4, seed=31000, trace="reduced")),
    ((0, 4, 1, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0), case("board", N=2, chains=33, steps=315, init="latin", sched=(COLD,), lanes=4, seed=32000, patience=25)),
    ((0, 4, 1, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0), case("board", N=3, chains=33, steps=333, init="random", sched=(LIN,), lanes=4, seed=33070, patience=200)),
    ((0, 4, 1, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0), case("board", N=4, chains=33, steps=389, init="random", sched=(COLD,), lanes=4, seed=34063, patience=120)),
    ((0, 4, 0, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=6, chains=33, steps=470, init="latin", sched=(CONST,), lanes=4, seed=35000)),
    ((0, 4, 0, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=8, chains=33, steps=315, init="klarner", sched=(LIN,), lanes=4, seed=36000)),
    ((0, 4, 0, 2, 0, 0, 0, 0, 1, 0, 0, 0, 0), case("board", N=5, chains=33, steps=333, init="random", sched=(EXP,), lanes=4, seed=37000)),
    ((0, 4, 0, 2, 1, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=5, chains=32, steps=389, init="latin", sched=(LOG, SIN), lanes=4, seed=38000, trace="reduced", inits=("latin", "klarner"))),
    ((0, 4, 0, 2, 1, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=8, chains=33, steps=470, init="klarner", sched=(SIN,), lanes=4, seed=39000, trace="reduced")),
    ((0, 4, 1, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=6, chains=33, steps=315, init="random", sched=(COLD,), lanes=4, seed=40021, patience=60)),
    ((0, 4, 1, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=8, chains=33, steps=333, init="latin", sched=(COLD,), lanes=4, seed=41000, patience=25)),
    ((0, 4, 1, 2, 0, 0, 0, 0, 1, 0, 0, 0, 0), case("board", N=5, chains=33, steps=389, init="klarner", sched=(COLD,), lanes=4, seed=42021, patience=60)),
    ((0, 4, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=9, chains=33, steps=470, init="random", sched=(LOG,), lanes=4, seed=43000)),
    ((0, 4, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=11, chains=33, steps=315, init="latin", sched=(SIN,), lanes=4, seed=44000)),
    ((0, 4, 0, 3, 1, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=9, chains=32, steps=333, init="klarner", sched=(CONST, LIN), lanes=4, seed=45000, trace="reduced", inits=("klarner", "random"))),
    ((0, 4, 0, 3, 1, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=11, chains=33, steps=389, init="random", sched=(LIN,), lanes=4, seed=46000, trace="reduced")),
    ((0, 4, 1, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=9, chains=33, steps=470, init="random", sched=(LIN,), lanes=4, seed=47014, patience=40)),
    ((0, 4, 1, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=11, chains=33, steps=315, init="random", sched=(CONST,), lanes=4, seed=48007, patience=40)),
    ((0, 4, 0, 3, 0, 0, 12, 0, 0, 0, 0, 0, 0), case("board", N=12, chains=33, steps=333, init="random", sched=(SIN,), lanes=4, seed=49000)),
    ((0, 4, 0, 3, 1, 0, 12, 0, 0, 0, 0, 0, 0), case("board", N=12, chains=32, steps=389, init="latin", sched=(CONST, LIN), lanes=4, seed=50000, trace="reduced", inits=("latin", "klarner"))),
    ((0, 4, 0, 3, 1, 0, 12, 0, 0, 0, 0, 0, 0), case("board", N=12, chains=33, steps=470, init="klarner", sched=(LIN,), lanes=4, seed=51000, trace="reduced")),
    ((0, 4, 1, 3, 0, 0, 12, 0, 0, 0, 0, 0, 0), case("board", N=12, chains=33, steps=315, init="random", sched=(COLD,), lanes=4, seed=52000, patience=25)),
    ((0, 4, 0, 4, 0, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=13, chains=33, steps=333, init="latin", sched=(LOG,), lanes=4, seed=53000)),
    ((0, 4, 0, 4, 0, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=16, chains=33, steps=389, init="klarner", sched=(SIN,), lanes=4, seed=54000)),
    ((0, 4, 0, 5, 0, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=19, chains=33, steps=470, init="random", sched=(CONST,), lanes=4, seed=55000)),
    ((0, 4, 0, 5, 0, 0, 17, 0, 0, 0, 0, 0, 0), case("board", N=17, chains=33, steps=315, init="latin", sched=(LIN,), lanes=4, seed=56000)),
    ((0, 4, 0, 5, 0, 0, 18, 0, 0, 0, 0, 0, 0), case("board", N=18, chains=33, steps=333, init="klarner", sched=(EXP,), lanes=4, seed=57000)),
    ((0, 4, 0, 5, 0, 0, 20, 0, 0, 0, 0, 0, 0), case("board", N=20, chains=33, steps=389, init="random", sched=(LOG,), lanes=4, seed=58000)),
    ((0, 4, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=21, chains=33, steps=470, init="latin", sched=(SIN,), lanes=4, seed=59000)),
    ((0, 4, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=24, chains=33, steps=315, init="klarner", sched=(CONST,), lanes=4, seed=60000)),
    ((0, 4, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=25, chains=33, steps=333, init="random", sched=(LIN,), lanes=4, seed=61000)),
    ((0, 4, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=98, chains=33, steps=389, init="latin", sched=(EXP,), lanes=4, seed=62000)),
    ((0, 4, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=13, chains=32, steps=470, init="klarner", sched=(LOG, SIN), lanes=4, seed=63000, trace="reduced", inits=("klarner", "random"))),
    ((0, 4, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=98, chains=33, steps=315, init="random", sched=(SIN,), lanes=4, seed=64000, trace="reduced")),
    ((0, 4, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=13, chains=33, steps=333, init="random", sched=(LIN,), lanes=4, seed=65014, patience=40)),
    ((0, 4, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=98, chains=33, steps=389, init="random", sched=(WARM,), lanes=4, seed=66028, patience=15)),
    ((0, 4, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=2, chains=32, steps=470, init="random", sched=(COLD, LOG), lanes=4, seed=67000, patience=25, trace="reduced", inits=("random", "latin"))),
    ((0, 4, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=3, chains=33, steps=315, init="klarner", sched=(LIN,), lanes=4, seed=68070, patience=200, trace="reduced")),
    ((0, 4, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=98, chains=33, steps=333, init="random", sched=(WARM,), lanes=4, seed=69028, patience=15, trace="reduced")),
    ((0, 8, 0, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=9, chains=17, steps=389, init="random", sched=(CONST,), lanes=8, seed=70000)),
    ((0, 8, 0, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=16, chains=17, steps=470, init="latin", sched=(LIN,), lanes=8, seed=71000)),
    ((0, 8, 0, 2, 1, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=9, chains=32, steps=315, init="klarner", sched=(EXP, LOG), lanes=8, seed=72000, trace="reduced", inits=("klarner", "random"))),
    ((0, 8, 0, 2, 1, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=16, chains=17, steps=333, init="random", sched=(LOG,), lanes=8, seed=73000, trace="reduced")),
    ((0, 8, 1, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=9, chains=17, steps=389, init="latin", sched=(COLD,), lanes=8, seed=74000, patience=25)),
    ((0, 8, 1, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=16, chains=17, steps=470, init="random", sched=(CONST,), lanes=8, seed=75007, patience=40)),
    ((0, 8, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=17, chains=16385, steps=301, init="random", sched=(LIN,), lanes=8, seed=76000)),
    ((0, 8, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=24, chains=16385, steps=301, init="latin", sched=(EXP,), lanes=8, seed=77000)),
    ((0, 8, 0, 3, 0, 0, 0, 0, 0, 1, 0, 0, 0), case("board", N=17, chains=17, steps=389, init="klarner", sched=(LOG,), lanes=8, seed=78000)),
    ((0, 8, 0, 3, 0, 0, 0, 0, 0, 1, 0, 0, 0), case("board", N=24, chains=17, steps=470, init="random", sched=(SIN,), lanes=8, seed=79000)),
    ((0, 8, 0, 3, 1, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=17, chains=16385, steps=301, init="latin", sched=(CONST,), lanes=8, seed=80000, trace="reduced")),
    ((0, 8, 0, 3, 1, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=23, chains=16385, steps=301, init="klarner", sched=(LIN,), lanes=8, seed=81000, trace="reduced")),
    ((0, 8, 0, 3, 1, 0, 0, 0, 0, 1, 0, 0, 0), case("board", N=17, chains=32, steps=389, init="random", sched=(EXP, LOG), lanes=8, seed=82000, trace="reduced", inits=("random", "latin"))),
    ((0, 8, 0, 3, 1, 0, 0, 0, 0, 1, 0, 0, 0), case("board", N=23, chains=17, steps=470, init="latin", sched=(LOG,), lanes=8, seed=83000, trace="reduced")),
    ((0, 8, 1, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=17, chains=16385, steps=301, init="random", sched=(CONST,), lanes=8, seed=84007, patience=40)),
    ((0, 8, 1, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=24, chains=16385, steps=301, init="random", sched=(COLD,), lanes=8, seed=85000, patience=25)),
    ((0, 8, 1, 3, 0, 0, 0, 0, 0, 1, 0, 0, 0), case("board", N=17, chains=17, steps=389, init="random", sched=(WARM,), lanes=8, seed=86056, patience=40)),
    ((0, 8, 1, 3, 0, 0, 0, 0, 0, 1, 0, 0, 0), case("board", N=24, chains=17, steps=470, init="random", sched=(CONST,), lanes=8, seed=87007, patience=40)),
    ((0, 8, 0, 3, 1, 0, 24, 0, 0, 0, 0, 0, 0), case("board", N=24, chains=16385, steps=301, init="random", sched=(LOG,), lanes=8, seed=88000, trace="reduced")),
    ((0, 8, 0, 3, 1, 0, 24, 0, 0, 1, 0, 0, 0), case("board", N=24, chains=32, steps=333, init="latin", sched=(SIN, CONST), lanes=8, seed=89000, trace="reduced", inits=("latin", "klarner"))),
    ((0, 8, 0, 3, 1, 0, 24, 0, 0, 1, 0, 0, 0), case("board", N=24, chains=17, steps=389, init="klarner", sched=(CONST,), lanes=8, seed=90000, trace="reduced")),
    ((0, 8, 0, 4, 0, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=25, chains=17, steps=470, init="random", sched=(LIN,), lanes=8, seed=91000)),
    ((0, 8, 0, 4, 0, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=32, chains=17, steps=315, init="latin", sched=(EXP,), lanes=8, seed=92000)),
    ((0, 8, 1, 4, 0, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=25, chains=17, steps=333, init="klarner", sched=(COLD,), lanes=8, seed=93021, patience=60)),
    ((0, 8, 1, 4, 0, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=32, chains=17, steps=389, init="klarner", sched=(LIN,), lanes=8, seed=94035, patience=90)),
    ((0, 8, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=2, chains=17, steps=470, init="latin", sched=(CONST,), lanes=8, seed=95000)),
    ((0, 8, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=3, chains=17, steps=315, init="klarner", sched=(LIN,), lanes=8, seed=96000)),
    ((0, 8, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=128, chains=17, steps=333, init="random", sched=(EXP,), lanes=8, seed=97000)),
    ((0, 8, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=2, chains=32, steps=389, init="latin", sched=(LOG, SIN), lanes=8, seed=98000, trace="reduced", inits=("latin", "klarner"))),
    ((0, 8, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=3, chains=17, steps=470, init="klarner", sched=(SIN,), lanes=8, seed=99000, trace="reduced")),
    ((0, 8, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=128, chains=17, steps=315, init="random", sched=(CONST,), lanes=8, seed=100000, trace="reduced")),
    ((0, 8, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=2, chains=17, steps=333, init="latin", sched=(COLD,), lanes=8, seed=101000, patience=25)),
    ((0, 8, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=3, chains=17, steps=389, init="random", sched=(LIN,), lanes=8, seed=102070, patience=200)),
    ((0, 8, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=128, chains=17, steps=470, init="random", sched=(COLD,), lanes=8, seed=103042, patience=12)),
    ((0, 8, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=2, chains=32, steps=315, init="latin", sched=(COLD, CONST), lanes=8, seed=104000, patience=25, trace="reduced", inits=("latin", "klarner"))),
    ((0, 8, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=3, chains=17, steps=333, init="random", sched=(LIN,), lanes=8, seed=105070, patience=200, trace="reduced")),
    ((0, 8, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=128, chains=17, steps=389, init="random", sched=(COLD,), lanes=8, seed=106042, patience=12, trace="reduced")),
    ((0, 16, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=2, chains=9, steps=470, init="latin", sched=(EXP,), lanes=16, seed=107000)),
    ((0, 16, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=3, chains=9, steps=315, init="klarner", sched=(LOG,), lanes=16, seed=108000)),
    ((0, 16, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=16, chains=9, steps=333, init="random", sched=(SIN,), lanes=16, seed=109000)),
    ((0, 16, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=2, chains=32, steps=389, init="latin", sched=(CONST, LIN), lanes=16, seed=110000, trace="reduced", inits=("latin", "klarner"))),
    ((0, 16, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=3, chains=9, steps=470, init="klarner", sched=(LIN,), lanes=16, seed=111000, trace="reduced")),
    ((0, 16, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=16, chains=9, steps=315, init="random", sched=(EXP,), lanes=16, seed=112000, trace="reduced")),
    ((0, 16, 0, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=17, chains=8193, steps=301, init="latin", sched=(LOG,), lanes=16, seed=113000)),
    ((0, 16, 0, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=32, chains=8193, steps=301, init="klarner", sched=(SIN,), lanes=16, seed=114000)),
    ((0, 16, 0, 2, 0, 0, 0, 0, 0, 1, 0, 0, 0), case("board", N=17, chains=9, steps=470, init="random", sched=(CONST,), lanes=16, seed=115000)),
    ((0, 16, 0, 2, 0, 0, 0, 0, 0, 1, 0, 0, 0), case("board", N=32, chains=9, steps=315, init="latin", sched=(LIN,), lanes=16, seed=116000)),
    ((0, 16, 0, 2, 1, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=17, chains=32, steps=333, init="klarner", sched=(EXP, LOG), lanes=16, seed=117000, trace="reduced", inits=("klarner", "random"))),
    ((0, 16, 0, 2, 1, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=32, chains=9, steps=389, init="random", sched=(LOG,), lanes=16, seed=118000, trace="reduced")),
    ((0, 16, 0, 2, 1, 0, 24, 0, 0, 0, 0, 0, 0), case("board", N=24, chains=32, steps=470, init="latin", sched=(SIN, CONST), lanes=16, seed=119000, trace="reduced", inits=("latin", "klarner"))),
    ((0, 16, 0, 2, 1, 0, 24, 0, 0, 0, 0, 0, 0), case("board", N=24, chains=9, steps=315, init="klarner", sched=(CONST,), lanes=16, seed=120000, trace="reduced")),
    ((0, 16, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=33, chains=9, steps=333, init="random", sched=(LIN,), lanes=16, seed=121000)),
    ((0, 16, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=128, chains=9, steps=389, init="latin", sched=(EXP,), lanes=16, seed=122000)),
    ((0, 16, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=33, chains=32, steps=470, init="klarner", sched=(LOG, SIN), lanes=16, seed=123000, trace="reduced", inits=("klarner", "random"))),
    ((0, 16, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=128, chains=9, steps=315, init="random", sched=(SIN,), lanes=16, seed=124000, trace="reduced")),
    ((0, 16, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=2, chains=9, steps=333, init="latin", sched=(COLD,), lanes=16, seed=125000, patience=25)),
    ((0, 16, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=3, chains=9, steps=389, init="random", sched=(LIN,), lanes=16, seed=126070, patience=200)),
    ((0, 16, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=128, chains=9, steps=470, init="random", sched=(COLD,), lanes=16, seed=127042, patience=12)),
    ((0, 16, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=2, chains=32, steps=315, init="latin", sched=(COLD, SIN), lanes=16, seed=128000, patience=25, trace="reduced", inits=("latin", "klarner"))),
    ((0, 16, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=3, chains=9, steps=333, init="random", sched=(LIN,), lanes=16, seed=129070, patience=200, trace="reduced")),
    ((0, 16, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0), case("board", N=128, chains=9, steps=389, init="klarner", sched=(LIN,), lanes=16, seed=130035, patience=90, trace="reduced")),
    ((1, 8, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0), case("full_3d", N=2, chains=17, steps=470, init="latin", sched=(LIN,), lanes=8, seed=131000)),
    ((1, 8, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0), case("full_3d", N=3, chains=17, steps=315, init="klarner", sched=(EXP,), lanes=8, seed=132000)),
    ((1, 8, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0), case("full_3d", N=4, chains=17, steps=333, init="random", sched=(LOG,), lanes=8, seed=133000)),
    ((1, 8, 0, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0), case("full_3d", N=5, chains=17, steps=389, init="latin", sched=(SIN,), lanes=8, seed=134000)),
    ((1, 8, 0, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0), case("full_3d", N=8, chains=17, steps=470, init="klarner", sched=(CONST,), lanes=8, seed=135000)),
    ((1, 8, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0), case("full_3d", N=9, chains=17, steps=315, init="random", sched=(LIN,), lanes=8, seed=136000)),
    ((1, 8, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0), case("full_3d", N=12, chains=17, steps=333, init="random", sched=(EXP,), lanes=8, seed=137000, Q=157)),
    ((1, 8, 0, 3, 1, 0, 0, 0, 0, 0, 0, 0, 0), case("full_3d", N=9, chains=32, steps=389, init="klarner", sched=(LOG, SIN), lanes=8, seed=138000, trace="reduced", inits=("klarner", "random"))),
    ((1, 8, 0, 3, 1, 0, 0, 0, 0, 0, 0, 0, 0), case("full_3d", N=12, chains=17, steps=470, init="random", sched=(SIN,), lanes=8, seed=139000, trace="reduced", Q=157)),
    ((1, 8, 0, 3, 0, 0, 12, 0, 0, 0, 0, 0, 0), case("full_3d", N=12, chains=17, steps=315, init="latin", sched=(CONST,), lanes=8, seed=140000)),
    ((1, 8, 0, 3, 1, 0, 12, 0, 0, 0, 0, 0, 0), case("full_3d", N=12, chains=32, steps=333, init="klarner", sched=(LIN, EXP), lanes=8, seed=141000, trace="reduced", inits=("klarner", "random"))),
    ((1, 8, 0, 3, 1, 0, 12, 0, 0, 0, 0, 0, 0), case("full_3d", N=12, chains=17, steps=389, init="random", sched=(EXP,), lanes=8, seed=142000, trace="reduced")),
    ((1, 8, 0, 4, 0, 0, 0, 0, 0, 0, 0, 0, 0), case("full_3d", N=13, chains=17, steps=470, init="latin", sched=(LOG,), lanes=8, seed=143000)),
    ((1, 8, 0, 4, 0, 0, 0, 0, 0, 0, 0, 0, 0), case("full_3d", N=16, chains=17, steps=315, init="klarner", sched=(SIN,), lanes=8, seed=144000)),
    ((1, 4, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0), case("full_3d", N=2, chains=33, steps=333, init="random", sched=(CONST,), lanes=4, seed=145000)),
    ((1, 4, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0), case("full_3d", N=3, chains=33, steps=389, init="latin", sched=(LIN,), lanes=4, seed=146000)),
    ((1, 4, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0), case("full_3d", N=32, chains=33, steps=470, init="klarner", sched=(EXP,), lanes=4, seed=147000)),
    ((1, 4, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0), case("full_3d", N=2, chains=32, steps=315, init="random", sched=(LOG, SIN), lanes=4, seed=148000, trace="reduced", inits=("random", "latin"))),
    ((1, 4, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0), case("full_3d", N=3, chains=33, steps=333, init="latin", sched=(SIN,), lanes=4, seed=149000, trace="reduced")),
    ((1, 4, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0), case("full_3d", N=32, chains=33, steps=389, init="klarner", sched=(CONST,), lanes=4, seed=150000, trace="reduced")),
    ((1, 8, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0), case("full_3d", N=17, chains=17, steps=470, init="random", sched=(LIN,), lanes=8, seed=151000)),
    ((1, 8, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0), case("full_3d", N=32, chains=17, steps=315, init="latin", sched=(EXP,), lanes=8, seed=152000)),
    ((1, 8, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0), case("full_3d", N=2, chains=32, steps=333, init="klarner", sched=(LOG, SIN), lanes=8, seed=153000, trace="reduced", inits=("klarner", "random"))),
    ((1, 8, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0), case("full_3d", N=3, chains=17, steps=389, init="random", sched=(SIN,), lanes=8, seed=154000, trace="reduced")),
    ((1, 8, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0), case("full_3d", N=32, chains=17, steps=470, init="latin", sched=(CONST,), lanes=8, seed=155000, trace="reduced")),
    ((1, 16, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0), case("full_3d", N=2, chains=9, steps=315, init="klarner", sched=(LIN,), lanes=16, seed=156000)),
    ((1, 16, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0), case("full_3d", N=3, chains=9, steps=333, init="random", sched=(EXP,), lanes=16, seed=157000)),
    ((1, 16, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0), case("full_3d", N=32, chains=9, steps=389, init="latin", sched=(LOG,), lanes=16, seed=158000)),
    ((1, 16, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0), case("full_3d", N=2, chains=32, steps=470, init="klarner", sched=(SIN, CONST), lanes=16, seed=159000, trace="reduced", inits=("klarner", "random"))),
    ((1, 16, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0), case("full_3d", N=3, chains=9, steps=315, init="random", sched=(CONST,), lanes=16, seed=160000, trace="reduced")),
    ((1, 16, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0), case("full_3d", N=32, chains=9, steps=333, init="latin", sched=(LIN,), lanes=16, seed=161000, trace="reduced")),
    ((1, 4, 0, 5, 0, 0, 0, 0, 0, 0, 1, 0, 0), case("full_3d", N=9, chains=33, steps=389, init="klarner", sched=(EXP,), lanes=4, seed=162000)),
    ((1, 4, 0, 5, 0, 0, 0, 0, 0, 0, 1, 0, 0), case("full_3d", N=10, chains=33, steps=470, init="random", sched=(LOG,), lanes=4, seed=163000)),
    ((1, 4, 0, 5, 0, 0, 0, 0, 0, 0, 1, 0, 0), case("full_3d", N=10, chains=33, steps=315, init="random", sched=(SIN,), lanes=4, seed=164000, Q=113)),
    ((1, 4, 0, 5, 1, 0, 0, 0, 0, 0, 1, 0, 0), case("full_3d", N=9, chains=32, steps=333, init="klarner", sched=(CONST, LIN), lanes=4, seed=165000, trace="reduced", inits=("klarner", "random"))),
    ((1, 4, 0, 5, 1, 0, 0, 0, 0, 0, 1, 0, 0), case("full_3d", N=10, chains=33, steps=389, init="random", sched=(LIN,), lanes=4, seed=166000, trace="reduced")),
    ((1, 4, 0, 5, 1, 0, 0, 0, 0, 0, 1, 0, 0), case("full_3d", N=10, chains=33, steps=470, init="random", sched=(EXP,), lanes=4, seed=167000, trace="reduced", Q=113)),
    ((1, 4, 0, 6, 0, 0, 0, 0, 0, 0, 1, 0, 0), case("full_3d", N=11, chains=33, steps=315, init="klarner", sched=(LOG,), lanes=4, seed=168000)),
    ((1, 4, 0, 6, 0, 0, 0, 0, 0, 0, 1, 0, 0), case("full_3d", N=12, chains=33, steps=333, init="random", sched=(SIN,), lanes=4, seed=169000, Q=157)),
    ((1, 4, 0, 6, 1, 0, 0, 0, 0, 0, 1, 0, 0), case("full_3d", N=11, chains=32, steps=389, init="latin", sched=(CONST, LIN), lanes=4, seed=170000, trace="reduced", inits=("latin", "klarner"))),
    ((1, 4, 0, 6, 1, 0, 0, 0, 0, 0, 1, 0, 0), case("full_3d", N=12, chains=33, steps=470, init="random", sched=(LIN,), lanes=4, seed=171000, trace="reduced", Q=157)),
    ((1, 4, 0, 6, 0, 0, 12, 0, 0, 0, 1, 0, 0), case("full_3d", N=12, chains=33, steps=315, init="random", sched=(EXP,), lanes=4, seed=172000)),
    ((1, 4, 0, 6, 1, 0, 12, 0, 0, 0, 1, 0, 0), case("full_3d", N=12, chains=32, steps=333, init="latin", sched=(LOG, SIN), lanes=4, seed=173000, trace="reduced", inits=("latin", "klarner"))),
    ((1, 4, 0, 6, 1, 0, 12, 0, 0, 0, 1, 0, 0), case("full_3d", N=12, chains=33, steps=389, init="klarner", sched=(SIN,), lanes=4, seed=174000, trace="reduced")),
    ((1, 16, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1), case("full_3d", N=33, chains=5, steps=470, init="random", sched=(CONST,), lanes=16, seed=175000)),
    ((1, 16, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1), case("full_3d", N=64, chains=5, steps=315, init="latin", sched=(LIN,), lanes=16, seed=176000)),
    ((1, 16, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 1), case("full_3d", N=33, chains=32, steps=333, init="klarner", sched=(EXP, LOG), lanes=16, seed=177000, trace="reduced", inits=("klarner", "random"))),
    ((1, 16, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 1), case("full_3d", N=64, chains=5, steps=389, init="random", sched=(LOG,), lanes=16, seed=178000, trace="reduced")),
    ((0, 4, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0), case("board", N=6, chains=33, steps=470, init="latin", sched=(SIN,), lanes=4, seed=179000, flags=CNT)),
    ((0, 4, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0), case("board", N=8, chains=33, steps=315, init="klarner", sched=(CONST,), lanes=4, seed=180000, flags=CNT)),
    ((0, 4, 0, 0, 0, 0, 0, 0, 1, 0, 0, 1, 0), case("board", N=2, chains=33, steps=333, init="random", sched=(LIN,), lanes=4, seed=181000, flags=CNT)),
    ((0, 4, 0, 0, 0, 0, 0, 0, 1, 0, 0, 1, 0), case("board", N=3, chains=33, steps=389, init="latin", sched=(EXP,), lanes=4, seed=182000, flags=CNT)),
    ((0, 4, 0, 0, 0, 0, 0, 0, 1, 0, 0, 1, 0), case("board", N=5, chains=33, steps=470, init="klarner", sched=(LOG,), lanes=4, seed=183000, flags=CNT)),
    ((0, 4, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0), case("board", N=6, chains=33, steps=315, init="klarner", sched=(LIN,), lanes=4, seed=184014, patience=40, flags=CNT)),
    ((0, 4, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0), case("board", N=8, chains=33, steps=333, init="latin", sched=(COLD,), lanes=4, seed=185000, patience=25, flags=CNT)),
    ((0, 4, 1, 0, 0, 0, 0, 0, 1, 0, 0, 1, 0), case("board", N=2, chains=33, steps=389, init="klarner", sched=(COLD,), lanes=4, seed=186000, patience=25, flags=CNT)),
    ((0, 4, 1, 0, 0, 0, 0, 0, 1, 0, 0, 1, 0), case("board", N=3, chains=33, steps=470, init="random", sched=(SIN,), lanes=4, seed=187084, patience=300, flags=CNT)),
    ((0, 4, 1, 0, 0, 0, 0, 0, 1, 0, 0, 1, 0), case("board", N=5, chains=33, steps=315, init="latin", sched=(COLD,), lanes=4, seed=188021, patience=60, flags=CNT)),
    ((0, 2, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0), case("board", N=2, chains=65, steps=333, init="klarner", sched=(SIN,), lanes=2, seed=189000, rng="philox")),
    ((0, 2, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0), case("board", N=3, chains=65, steps=389, init="random", sched=(CONST,), lanes=2, seed=190000, rng="philox")),
    ((0, 2, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0), case("board", N=67, chains=65, steps=470, init="latin", sched=(LIN,), lanes=2, seed=191000, rng="philox")),
    ((0, 2, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0), case("board", N=2, chains=64, steps=315, init="klarner", sched=(EXP, LOG), lanes=2, seed=192000, trace="reduced", rng="philox", inits=("klarner", "random"))),
    ((0, 2, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0), case("board", N=3, chains=65, steps=333, init="random", sched=(LOG,), lanes=2, seed=193000, trace="reduced", rng="philox")),
    ((0, 2, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0), case("board", N=67, chains=65, steps=389, init="latin", sched=(SIN,), lanes=2, seed=194000, trace="reduced", rng="philox")),
    ((0, 2, 1, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0), case("board", N=2, chains=65, steps=470, init="klarner", sched=(COLD,), lanes=2, seed=195000, patience=25, rng="philox")),
    ((0, 2, 1, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0), case("board", N=3, chains=65, steps=315, init="latin", sched=(LIN,), lanes=2, seed=196070, patience=200, rng="philox")),
    ((0, 2, 1, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0), case("board", N=67, chains=65, steps=333, init="random", sched=(WARM,), lanes=2, seed=197056, patience=40, rng="philox")),
    ((0, 2, 1, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0), case("board", N=2, chains=64, steps=389, init="klarner", sched=(COLD, SIN), lanes=2, seed=198000, patience=25, trace="reduced", rng="philox", inits=("klarner", "random"))),
    ((0, 2, 1, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0), case("board", N=3, chains=65, steps=470, init="random", sched=(SIN,), lanes=2, seed=199084, patience=300, trace="reduced", rng="philox")),
    ((0, 2, 1, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0), case("board", N=67, chains=65, steps=315, init="random", sched=(WARM,), lanes=2, seed=200056, patience=40, trace="reduced", rng="philox")),
    ((0, 4, 0, 3, 0, 1, 0, 0, 0, 0, 0, 0, 0), case("board", N=9, chains=33, steps=333, init="klarner", sched=(LIN,), lanes=4, seed=201000, rng="philox")),
    ((0, 4, 0, 3, 0, 1, 0, 0, 0, 0, 0, 0, 0), case("board", N=11, chains=33, steps=389, init="random", sched=(EXP,), lanes=4, seed=202000, rng="philox")),
    ((0, 4, 0, 3, 0, 1, 12, 0, 0, 0, 0, 0, 0), case("board", N=12, chains=33, steps=470, init="latin", sched=(LOG,), lanes=4, seed=203000, rng="philox")),
    ((0, 4, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0), case("board", N=2, chains=33, steps=315, init="klarner", sched=(SIN,), lanes=4, seed=204000, rng="philox")),
    ((0, 4, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0), case("board", N=3, chains=33, steps=333, init="random", sched=(CONST,), lanes=4, seed=205000, rng="philox")),
    ((0, 4, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0), case("board", N=98, chains=33, steps=389, init="latin", sched=(LIN,), lanes=4, seed=206000, rng="philox")),
    ((0, 4, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0), case("board", N=2, chains=32, steps=470, init="klarner", sched=(EXP, LOG), lanes=4, seed=207000, trace="reduced", rng="philox", inits=("klarner", "random"))),
    ((0, 4, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0), case("board", N=3, chains=33, steps=315, init="random", sched=(LOG,), lanes=4, seed=208000, trace="reduced", rng="philox")),
    ((0, 4, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0), case("board", N=98, chains=33, steps=333, init="latin", sched=(SIN,), lanes=4, seed=209000, trace="reduced", rng="philox")),
    ((0, 4, 1, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0), case("board", N=2, chains=33, steps=389, init="klarner", sched=(COLD,), lanes=4, seed=210000, patience=25, rng="philox")),
    ((0, 4, 1, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0), case("board", N=3, chains=33, steps=470, init="random", sched=(SIN,), lanes=4, seed=211084, patience=300, rng="philox")),
    ((0, 4, 1, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0), case("board", N=98, chains=33, steps=315, init="klarner", sched=(LIN,), lanes=4, seed=212070, patience=200, rng="philox")),
    ((0, 4, 1, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0), case("board", N=2, chains=32, steps=333, init="klarner", sched=(COLD, SIN), lanes=4, seed=213000, patience=25, trace="reduced", rng="philox", inits=("klarner", "random"))),
    ((0, 4, 1, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0), case("board", N=3, chains=33, steps=389, init="latin", sched=(LIN,), lanes=4, seed=214070, patience=200, trace="reduced", rng="philox")),
    ((0, 4, 1, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0), case("board", N=98, chains=33, steps=470, init="klarner", sched=(LIN,), lanes=4, seed=215070, patience=200, trace="reduced", rng="philox")),
    ((0, 8, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0), case("board", N=2, chains=17, steps=315, init="klarner", sched=(LIN,), lanes=8, seed=216000, rng="philox")),
    ((0, 8, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0), case("board", N=3, chains=17, steps=333, init="random", sched=(EXP,), lanes=8, seed=217000, rng="philox")),
    ((0, 8, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0), case("board", N=128, chains=17, steps=389, init="latin", sched=(LOG,), lanes=8, seed=218000, rng="philox")),
    ((0, 8, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0), case("board", N=2, chains=32, steps=470, init="klarner", sched=(SIN, CONST), lanes=8, seed=219000, trace="reduced", rng="philox", inits=("klarner", "random"))),
    ((0, 8, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0), case("board", N=3, chains=17, steps=315, init="random", sched=(CONST,), lanes=8, seed=220000, trace="reduced", rng="philox")),
    ((0, 8, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0), case("board", N=128, chains=17, steps=333, init="latin", sched=(LIN,), lanes=8, seed=221000, trace="reduced", rng="philox")),
    ((0, 8, 1, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0), case("board", N=2, chains=17, steps=389, init="klarner", sched=(COLD,), lanes=8, seed=222000, patience=25, rng="philox")),
    ((0, 8, 1, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0), case("board", N=3, chains=17, steps=470, init="random", sched=(SIN,), lanes=8, seed=223084, patience=300, rng="philox")),
    ((0, 8, 1, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0), case("board", N=128, chains=17, steps=315, init="klarner", sched=(LIN,), lanes=8, seed=224070, patience=200, rng="philox")),
    ((0, 8, 1, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0), case("board", N=2, chains=32, steps=333, init="klarner", sched=(COLD, LIN), lanes=8, seed=225000, patience=25, trace="reduced", rng="philox", inits=("klarner", "random"))),
    ((0, 8, 1, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0), case("board", N=3, chains=17, steps=389, init="latin", sched=(LIN,), lanes=8, seed=226070, patience=200, trace="reduced", rng="philox")),
    ((0, 8, 1, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0), case("board", N=128, chains=17, steps=470, init="klarner", sched=(LIN,), lanes=8, seed=227070, patience=200, trace="reduced", rng="philox")),
    ((0, 16, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0), case("board", N=2, chains=9, steps=315, init="klarner", sched=(LOG,), lanes=16, seed=228000, rng="philox")),
    ((0, 16, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0), case("board", N=3, chains=9, steps=333, init="random", sched=(SIN,), lanes=16, seed=229000, rng="philox")),
    ((0, 16, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0), case("board", N=128, chains=9, steps=389, init="latin", sched=(CONST,), lanes=16, seed=230000, rng="philox")),
    ((0, 16, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0), case("board", N=2, chains=32, steps=470, init="klarner", sched=(LIN, EXP), lanes=16, seed=231000, trace="reduced", rng="philox", inits=("klarner", "random"))),
    ((0, 16, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0), case("board", N=3, chains=9, steps=315, init="random", sched=(EXP,), lanes=16, seed=232000, trace="reduced", rng="philox")),
    ((0, 16, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0), case("board", N=128, chains=9, steps=333, init="latin", sched=(LOG,), lanes=16, seed=233000, trace="reduced", rng="philox")),
    ((0, 16, 1, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0), case("board", N=2, chains=9, steps=389, init="klarner", sched=(COLD,), lanes=16, seed=234000, patience=25, rng="philox")),
    ((0, 16, 1, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0), case("board", N=3, chains=9, steps=470, init="latin", sched=(EXP,), lanes=16, seed=235091, patience=290, rng="philox")),
    ((0, 16, 1, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0), case("board", N=128, chains=9, steps=315, init="klarner", sched=(LIN,), lanes=16, seed=236070, patience=200, rng="philox")),
    ((0, 16, 1, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0), case("board", N=2, chains=32, steps=333, init="klarner", sched=(COLD, LOG), lanes=16, seed=237000, patience=25, trace="reduced", rng="philox", inits=("klarner", "random"))),
    ((0, 16, 1, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0), case("board", N=3, chains=9, steps=389, init="latin", sched=(LIN,), lanes=16, seed=238070, patience=200, trace="reduced", rng="philox")),
    ((0, 16, 1, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0), case("board", N=128, chains=9, steps=470, init="klarner", sched=(EXP,), lanes=16, seed=239091, patience=290, trace="reduced", rng="philox")),
    ((1, 4, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0), case("full_3d", N=2, chains=33, steps=315, init="klarner", sched=(CONST,), lanes=4, seed=240000, rng="philox")),
    ((1, 4, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0), case("full_3d", N=3, chains=33, steps=333, init="random", sched=(LIN,), lanes=4, seed=241000, rng="philox")),
    ((1, 4, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0), case("full_3d", N=32, chains=33, steps=389, init="latin", sched=(EXP,), lanes=4, seed=242000, rng="philox")),
    ((1, 4, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0), case("full_3d", N=2, chains=32, steps=470, init="klarner", sched=(LOG, SIN), lanes=4, seed=243000, trace="reduced", rng="philox", inits=("klarner", "random"))),
    ((1, 4, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0), case("full_3d", N=3, chains=33, steps=315, init="random", sched=(SIN,), lanes=4, seed=244000, trace="reduced", rng="philox")),
    ((1, 4, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0), case("full_3d", N=32, chains=33, steps=333, init="latin", sched=(CONST,), lanes=4, seed=245000, trace="reduced", rng="philox")),
    ((1, 8, 0, 3, 0, 1, 0, 0, 0, 0, 0, 0, 0), case("full_3d", N=9, chains=17, steps=389, init="klarner", sched=(LIN,), lanes=8, seed=246000, rng="philox")),
    ((1, 8, 0, 3, 0, 1, 0, 0, 0, 0, 0, 0, 0), case("full_3d", N=12, chains=17, steps=470, init="random", sched=(EXP,), lanes=8, seed=247000, rng="philox", Q=157)),
    ((1, 8, 0, 3, 0, 1, 12, 0, 0, 0, 0, 0, 0), case("full_3d", N=12, chains=17, steps=315, init="latin", sched=(LOG,), lanes=8, seed=248000, rng="philox")),
    ((1, 8, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0), case("full_3d", N=2, chains=17, steps=333, init="klarner", sched=(SIN,), lanes=8, seed=249000, rng="philox")),
    ((1, 8, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0), case("full_3d", N=3, chains=17, steps=389, init="random", sched=(CONST,), lanes=8, seed=250000, rng="philox")),
    ((1, 8, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0), case("full_3d", N=32, chains=17, steps=470, init="latin", sched=(LIN,), lanes=8, seed=251000, rng="philox")),
    ((1, 8, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0), case("full_3d", N=2, chains=32, steps=315, init="klarner", sched=(EXP, LOG), lanes=8, seed=252000, trace="reduced", rng="philox", inits=("klarner", "random"))),
    ((1, 8, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0), case("full_3d", N=3, chains=17, steps=333, init="random", sched=(LOG,), lanes=8, seed=253000, trace="reduced", rng="philox")),
    ((1, 8, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0), case("full_3d", N=32, chains=17, steps=389, init="latin", sched=(SIN,), lanes=8, seed=254000, trace="reduced", rng="philox")),
    ((1, 16, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0), case("full_3d", N=2, chains=9, steps=470, init="klarner", sched=(CONST,), lanes=16, seed=255000, rng="philox")),
    ((1, 16, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0), case("full_3d", N=3, chains=9, steps=315, init="random", sched=(LIN,), lanes=16, seed=256000, rng="philox")),
    ((1, 16, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0), case("full_3d", N=32, chains=9, steps=333, init="latin", sched=(EXP,), lanes=16, seed=257000, rng="philox")),
    ((1, 16, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0), case("full_3d", N=2, chains=32, steps=389, init="klarner", sched=(LOG, SIN), lanes=16, seed=258000, trace="reduced", rng="philox", inits=("klarner", "random"))),
    ((1, 16, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0), case("full_3d", N=3, chains=9, steps=470, init="random", sched=(SIN,), lanes=16, seed=259000, trace="reduced", rng="philox")),
    ((1, 16, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0), case("full_3d", N=32, chains=9, steps=315, init="latin", sched=(CONST,), lanes=16, seed=260000, trace="reduced", rng="philox")),
    ((0, 2, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0), case("board", N=2, chains=80, steps=333, init="klarner", sched=(LIN,), lanes=2, seed=261000, exch=(7, 16, 0.7, 1.4))),
    ((0, 2, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0), case("board", N=3, chains=80, steps=389, init="random", sched=(EXP,), lanes=2, seed=262000, exch=(7, 16, 0.7, 1.4))),
    ((0, 2, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0), case("board", N=67, chains=80, steps=470, init="latin", sched=(LOG,), lanes=2, seed=263000, exch=(7, 16, 0.7, 1.4))),
    ((0, 2, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0), case("board", N=2, chains=66, steps=315, init="klarner", sched=(SIN,), lanes=2, seed=264000, exch=(3, 2, 0.7, 1.4))),
    ((0, 2, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0), case("board", N=3, chains=66, steps=333, init="random", sched=(CONST,), lanes=2, seed=265000, exch=(3, 2, 0.7, 1.4))),
    ((0, 2, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0), case("board", N=67, chains=66, steps=389, init="latin", sched=(LIN,), lanes=2, seed=266000, exch=(3, 2, 0.7, 1.4))),
    ((0, 2, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0, 0), case("board", N=2, chains=80, steps=470, init="klarner", sched=(EXP,), lanes=2, seed=267000, rng="philox", exch=(7, 16, 0.7, 1.4))),
    ((0, 2, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0, 0), case("board", N=3, chains=80, steps=315, init="random", sched=(LOG,), lanes=2, seed=268000, rng="philox", exch=(7, 16, 0.7, 1.4))),
    ((0, 2, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0, 0), case("board", N=67, chains=80, steps=333, init="latin", sched=(SIN,), lanes=2, seed=269000, rng="philox", exch=(7, 16, 0.7, 1.4))),
    ((0, 2, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0, 0), case("board", N=2, chains=66, steps=389, init="klarner", sched=(CONST,), lanes=2, seed=270000, rng="philox", exch=(3, 2, 0.7, 1.4))),
    ((0, 2, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0, 0), case("board", N=3, chains=66, steps=470, init="random", sched=(LIN,), lanes=2, seed=271000, rng="philox", exch=(3, 2, 0.7, 1.4))),
    ((0, 2, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0, 0), case("board", N=67, chains=66, steps=315, init="latin", sched=(EXP,), lanes=2, seed=272000, rng="philox", exch=(3, 2, 0.7, 1.4))),
    ((0, 4, 0, 3, 0, 0, 12, 1, 0, 0, 0, 0, 0), case("board", N=12, chains=48, steps=333, init="klarner", sched=(LOG,), lanes=4, seed=273000, exch=(7, 16, 0.7, 1.4))),
    ((0, 4, 0, 3, 0, 0, 12, 1, 0, 0, 0, 0, 0), case("board", N=12, chains=34, steps=389, init="random", sched=(SIN,), lanes=4, seed=274000, exch=(3, 2, 0.7, 1.4))),
    ((0, 4, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0), case("board", N=2, chains=48, steps=470, init="latin", sched=(CONST,), lanes=4, seed=275000, exch=(7, 16, 0.7, 1.4))),
    ((0, 4, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0), case("board", N=3, chains=48, steps=315, init="klarner", sched=(LIN,), lanes=4, seed=276000, exch=(7, 16, 0.7, 1.4))),
    ((0, 4, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0), case("board", N=98, chains=48, steps=333, init="random", sched=(EXP,), lanes=4, seed=277000, exch=(7, 16, 0.7, 1.4))),
    ((0, 4, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0), case("board", N=2, chains=34, steps=389, init="latin", sched=(LOG,), lanes=4, seed=278000, exch=(3, 2, 0.7, 1.4))),
    ((0, 4, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0), case("board", N=3, chains=34, steps=470, init="klarner", sched=(SIN,), lanes=4, seed=279000, exch=(3, 2, 0.7, 1.4))),
    ((0, 4, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0), case("board", N=98, chains=34, steps=315, init="random", sched=(CONST,), lanes=4, seed=280000, exch=(3, 2, 0.7, 1.4))),
    ((0, 4, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0, 0), case("board", N=2, chains=48, steps=333, init="latin", sched=(LIN,), lanes=4, seed=281000, rng="philox", exch=(7, 16, 0.7, 1.4))),
    ((0, 4, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0, 0), case("board", N=3, chains=48, steps=389, init="klarner", sched=(EXP,), lanes=4, seed=282000, rng="philox", exch=(7, 16, 0.7, 1.4))),
    ((0, 4, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0, 0), case("board", N=98, chains=48, steps=470, init="random", sched=(LOG,), lanes=4, seed=283000, rng="philox", exch=(7, 16, 0.7, 1.4))),
    ((0, 4, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0, 0), case("board", N=2, chains=34, steps=315, init="latin", sched=(SIN,), lanes=4, seed=284000, rng="philox", exch=(3, 2, 0.7, 1.4))),
    ((0, 4, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0, 0), case("board", N=3, chains=34, steps=333, init="klarner", sched=(CONST,), lanes=4, seed=285000, rng="philox", exch=(3, 2, 0.7, 1.4))),
    ((0, 4, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0, 0), case("board", N=98, chains=34, steps=389, init="random", sched=(LIN,), lanes=4, seed=286000, rng="philox", exch=(3, 2, 0.7, 1.4))),
    ((0, 8, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0), case("board", N=2, chains=24, steps=470, init="latin", sched=(EXP,), lanes=8, seed=287000, exch=(7, 8, 0.7, 1.4))),
    ((0, 8, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0), case("board", N=3, chains=24, steps=315, init="klarner", sched=(LOG,), lanes=8, seed=288000, exch=(7, 8, 0.7, 1.4))),
    ((0, 8, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0), case("board", N=128, chains=24, steps=333, init="random", sched=(SIN,), lanes=8, seed=289000, exch=(7, 8, 0.7, 1.4))),
    ((0, 8, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0), case("board", N=2, chains=18, steps=389, init="latin", sched=(CONST,), lanes=8, seed=290000, exch=(3, 2, 0.7, 1.4))),
    ((0, 8, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0), case("board", N=3, chains=18, steps=470, init="klarner", sched=(LIN,), lanes=8, seed=291000, exch=(3, 2, 0.7, 1.4))),
    ((0, 8, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0), case("board", N=128, chains=18, steps=315, init="random", sched=(EXP,), lanes=8, seed=292000, exch=(3, 2, 0.7, 1.4))),
    ((0, 8, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0, 0), case("board", N=2, chains=24, steps=333, init="latin", sched=(LOG,), lanes=8, seed=293000, rng="philox", exch=(7, 8, 0.7, 1.4))),
    ((0, 8, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0, 0), case("board", N=3, chains=24, steps=389, init="klarner", sched=(SIN,), lanes=8, seed=294000, rng="philox", exch=(7, 8, 0.7, 1.4))),
    ((0, 8, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0, 0), case("board", N=128, chains=24, steps=470, init="random", sched=(CONST,), lanes=8, seed=295000, rng="philox", exch=(7, 8, 0.7, 1.4))),
    ((0, 8, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0, 0), case("board", N=2, chains=18, steps=315, init="latin", sched=(LIN,), lanes=8, seed=296000, rng="philox", exch=(3, 2, 0.7, 1.4))),
    ((0, 8, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0, 0), case("board", N=3, chains=18, steps=333, init="klarner", sched=(EXP,), lanes=8, seed=297000, rng="philox", exch=(3, 2, 0.7, 1.4))),
    ((0, 8, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0, 0), case("board", N=128, chains=18, steps=389, init="random", sched=(LOG,), lanes=8, seed=298000, rng="philox", exch=(3, 2, 0.7, 1.4))),
    ((0, 16, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0), case("board", N=2, chains=12, steps=470, init="latin", sched=(SIN,), lanes=16, seed=299000, exch=(7, 4, 0.7, 1.4))),
    ((0, 16, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0), case("board", N=3, chains=12, steps=315, init="klarner", sched=(CONST,), lanes=16, seed=300000, exch=(7, 4, 0.7, 1.4))),
    ((0, 16, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0), case("board", N=128, chains=12, steps=333, init="random", sched=(LIN,), lanes=16, seed=301000, exch=(7, 4, 0.7, 1.4))),
    ((0, 16, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0), case("board", N=2, chains=10, steps=389, init="latin", sched=(EXP,), lanes=16, seed=302000, exch=(3, 2, 0.7, 1.4))),
    ((0, 16, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0), case("board", N=3, chains=10, steps=470, init="klarner", sched=(LOG,), lanes=16, seed=303000, exch=(3, 2, 0.7, 1.4))),
    ((0, 16, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0), case("board", N=128, chains=10, steps=315, init="latin", sched=(CONST,), lanes=16, seed=304007, exch=(3, 2, 0.7, 1.4))),
    ((0, 16, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0, 0), case("board", N=2, chains=12, steps=333, init="latin", sched=(CONST,), lanes=16, seed=305000, rng="philox", exch=(7, 4, 0.7, 1.4))),
    ((0, 16, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0, 0), case("board", N=3, chains=12, steps=389, init="klarner", sched=(LIN,), lanes=16, seed=306000, rng="philox", exch=(7, 4, 0.7, 1.4))),
    ((0, 16, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0, 0), case("board", N=128, chains=12, steps=470, init="random", sched=(EXP,), lanes=16, seed=307000, rng="philox", exch=(7, 4, 0.7, 1.4))),
    ((0, 16, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0, 0), case("board", N=2, chains=10, steps=315, init="latin", sched=(LOG,), lanes=16, seed=308000, rng="philox", exch=(3, 2, 0.7, 1.4))),
    ((0, 16, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0, 0), case("board", N=3, chains=10, steps=333, init="klarner", sched=(SIN,), lanes=16, seed=309000, rng="philox", exch=(3, 2, 0.7, 1.4))),
    ((0, 16, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0, 0), case("board", N=128, chains=10, steps=389, init="random", sched=(CONST,), lanes=16, seed=310000, rng="philox", exch=(3, 2, 0.7, 1.4))),
    ((1, 4, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0), case("full_3d", N=2, chains=48, steps=470, init="latin", sched=(LIN,), lanes=4, seed=311000, exch=(7, 16, 0.7, 1.4))),
    ((1, 4, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0), case("full_3d", N=3, chains=48, steps=315, init="klarner", sched=(EXP,), lanes=4, seed=312000, exch=(7, 16, 0.7, 1.4))),
    ((1, 4, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0), case("full_3d", N=32, chains=48, steps=333, init="random", sched=(LOG,), lanes=4, seed=313000, exch=(7, 16, 0.7, 1.4))),
    ((1, 4, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0), case("full_3d", N=2, chains=34, steps=389, init="latin", sched=(SIN,), lanes=4, seed=314000, exch=(3, 2, 0.7, 1.4))),
    ((1, 4, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0), case("full_3d", N=3, chains=34, steps=470, init="klarner", sched=(CONST,), lanes=4, seed=315000, exch=(3, 2, 0.7, 1.4))),
    ((1, 4, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0), case("full_3d", N=32, chains=34, steps=315, init="random", sched=(LIN,), lanes=4, seed=316000, exch=(3, 2, 0.7, 1.4))),
    ((1, 4, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0, 0), case("full_3d", N=2, chains=48, steps=333, init="latin", sched=(EXP,), lanes=4, seed=317000, rng="philox", exch=(7, 16, 0.7, 1.4))),
    ((1, 4, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0, 0), case("full_3d", N=3, chains=48, steps=389, init="klarner", sched=(LOG,), lanes=4, seed=318000, rng="philox", exch=(7, 16, 0.7, 1.4))),
    ((1, 4, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0, 0), case("full_3d", N=32, chains=48, steps=470, init="random", sched=(SIN,), lanes=4, seed=319000, rng="philox", exch=(7, 16, 0.7, 1.4))),
    ((1, 4, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0, 0), case("full_3d", N=2, chains=34, steps=315, init="latin", sched=(CONST,), lanes=4, seed=320000, rng="philox", exch=(3, 2, 0.7, 1.4))),
    ((1, 4, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0, 0), case("full_3d", N=3, chains=34, steps=333, init="klarner", sched=(LIN,), lanes=4, seed=321000, rng="philox", exch=(3, 2, 0.7, 1.4))),
    ((1, 4, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0, 0), case("full_3d", N=32, chains=34, steps=389, init="random", sched=(EXP,), lanes=4, seed=322000, rng="philox", exch=(3, 2, 0.7, 1.4))),
    ((1, 8, 0, 3, 0, 0, 12, 1, 0, 0, 0, 0, 0), case("full_3d", N=12, chains=24, steps=470, init="latin", sched=(LOG,), lanes=8, seed=323000, exch=(7, 8, 0.7, 1.4))),
    ((1, 8, 0, 3, 0, 0, 12, 1, 0, 0, 0, 0, 0), case("full_3d", N=12, chains=18, steps=315, init="klarner", sched=(SIN,), lanes=8, seed=324000, exch=(3, 2, 0.7, 1.4))),
    ((1, 8, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0), case("full_3d", N=2, chains=24, steps=333, init="random", sched=(CONST,), lanes=8, seed=325000, exch=(7, 8, 0.7, 1.4))),
    ((1, 8, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0), case("full_3d", N=3, chains=24, steps=389, init="latin", sched=(LIN,), lanes=8, seed=326000, exch=(7, 8, 0.7, 1.4))),
    ((1, 8, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0), case("full_3d", N=32, chains=24, steps=470, init="klarner", sched=(EXP,), lanes=8, seed=327000, exch=(7, 8, 0.7, 1.4))),
    ((1, 8, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0), case("full_3d", N=2, chains=18, steps=315, init="random", sched=(LOG,), lanes=8, seed=328000, exch=(3, 2, 0.7, 1.4))),
    ((1, 8, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0), case("full_3d", N=3, chains=18, steps=333, init="latin", sched=(SIN,), lanes=8, seed=329000, exch=(3, 2, 0.7, 1.4))),
    ((1, 8, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0), case("full_3d", N=32, chains=18, steps=389, init="klarner", sched=(CONST,), lanes=8, seed=330000, exch=(3, 2, 0.7, 1.4))),
    ((1, 8, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0, 0), case("full_3d", N=2, chains=24, steps=470, init="random", sched=(LIN,), lanes=8, seed=331000, rng="philox", exch=(7, 8, 0.7, 1.4))),
    ((1, 8, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0, 0), case("full_3d", N=3, chains=24, steps=315, init="latin", sched=(EXP,), lanes=8, seed=332000, rng="philox", exch=(7, 8, 0.7, 1.4))),
    ((1, 8, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0, 0), case("full_3d", N=32, chains=24, steps=333, init="klarner", sched=(LOG,), lanes=8, seed=333000, rng="philox", exch=(7, 8, 0.7, 1.4))),
    ((1, 8, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0, 0), case("full_3d", N=2, chains=18, steps=389, init="random", sched=(SIN,), lanes=8, seed=334000, rng="philox", exch=(3, 2, 0.7, 1.4))),
    ((1, 8, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0, 0), case("full_3d", N=3, chains=18, steps=470, init="latin", sched=(CONST,), lanes=8, seed=335000, rng="philox", exch=(3, 2, 0.7, 1.4))),
    ((1, 8, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0, 0), case("full_3d", N=32, chains=18, steps=315, init="klarner", sched=(LIN,), lanes=8, seed=336000, rng="philox", exch=(3, 2, 0.7, 1.4))),
    ((1, 16, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0), case("full_3d", N=2, chains=12, steps=333, init="random", sched=(EXP,), lanes=16, seed=337000, exch=(7, 4, 0.7, 1.4))),
    ((1, 16, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0), case("full_3d", N=3, chains=12, steps=389, init="latin", sched=(LOG,), lanes=16, seed=338000, exch=(7, 4, 0.7, 1.4))),
    ((1, 16, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0), case("full_3d", N=32, chains=12, steps=470, init="klarner", sched=(SIN,), lanes=16, seed=339000, exch=(7, 4, 0.7, 1.4))),
    ((1, 16, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0), case("full_3d", N=2, chains=10, steps=315, init="random", sched=(CONST,), lanes=16, seed=340000, exch=(3, 2, 0.7, 1.4))),
    ((1, 16, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0), case("full_3d", N=3, chains=10, steps=333, init="latin", sched=(LIN,), lanes=16, seed=341000, exch=(3, 2, 0.7, 1.4))),
    ((1, 16, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0), case("full_3d", N=32, chains=10, steps=389, init="klarner", sched=(EXP,), lanes=16, seed=342000, exch=(3, 2, 0.7, 1.4))),
    ((1, 16, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0, 0), case("full_3d", N=2, chains=12, steps=470, init="random", sched=(LOG,), lanes=16, seed=343000, rng="philox", exch=(7, 4, 0.7, 1.4))),
    ((1, 16, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0, 0), case("full_3d", N=3, chains=12, steps=315, init="latin", sched=(SIN,), lanes=16, seed=344000, rng="philox", exch=(7, 4, 0.7, 1.4))),
    ((1, 16, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0, 0), case("full_3d", N=32, chains=12, steps=333, init="klarner", sched=(CONST,), lanes=16, seed=345000, rng="philox", exch=(7, 4, 0.7, 1.4))),
    ((1, 16, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0, 0), case("full_3d", N=2, chains=10, steps=389, init="random", sched=(LIN,), lanes=16, seed=346000, rng="philox", exch=(3, 2, 0.7, 1.4))),
    ((1, 16, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0, 0), case("full_3d", N=3, chains=10, steps=470, init="latin", sched=(EXP,), lanes=16, seed=347000, rng="philox", exch=(3, 2, 0.7, 1.4))),
    ((1, 16, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0, 0), case("full_3d", N=32, chains=10, steps=315, init="klarner", sched=(LOG,), lanes=16, seed=348000, rng="philox", exch=(3, 2, 0.7, 1.4))),
    # --- table end
]


def reachable_rows():
    """The rows of SWEEP_TABLE a parameter block can select, in the table's order."""
    return [r for r in _table_rows() if r not in KNOWN_UNREACHED]


def cases_of(row):
    return [(i, c) for i, (r, c) in enumerate(CASES) if r == row]


def row_id(row):
    return "-".join(str(x) for x in row)


def ladder(exch):
    _, R, lo, hi = exch
    return lo * (hi / lo) ** (np.arange(R) / (R - 1))


def build(c, chains=None):
    """(params, seeds) of a case; `chains` overrides the chain count of a case without schedule sets."""
    mode = c["mode"]
    n = c["chains"] if chains is None else chains
    kw = dict(mcmc_type=mode, early_stop_patience=c["patience"], trace=c["trace"], flags=c["flags"], lanes_per_chain=c["lanes"], rng=c["rng"])
    if len(c["sched"]) > 1:
        assert chains is None and c["Q"] is None and n % len(c["sched"]) == 0
        cps = n // len(c["sched"])
        p = abi.make_params_sets(c["N"], c["steps"], c["init"], list(c["sched"]), cps, init_modes=None if c["inits"] is None else list(c["inits"]), **kw)
        seeds = np.concatenate([abi.seeds_for(c["seed"] + 1000 * t, cps) for t in range(len(c["sched"]))])
    else:
        p = abi.make_params(c["N"], c["steps"], c["init"], c["sched"][0], n, Q=c["Q"], **kw)
        seeds = abi.seeds_for(c["seed"], n)
    if c["exch"]:
        abi.set_exchange(p, c["exch"][0], ladder(c["exch"]))
    return p, seeds


def heavy(row, c):
    """The cases whose naive oracle run takes seconds (16 385 chains; boards beyond N = 64, where it recounts 2 N^2 cells per step): the
    tests take the fast oracle for them, and the CPU test holds the naive one to it on the first chain or ladder (prefix_chains)."""
    return row in LARGE_ROWS or (c["mode"] == "board" and c["N"] > 64 and len(c["sched"]) == 1)


def prefix_chains(c):
    return c["exch"][1] if c["exch"] else 1


def variant_of(p):
    """The row a launch with these parameters takes, as mcq_sweep_variant names it (no GPU needed)."""
    v = mcq_amd._lib.sweep_variant(p)
    return tuple(int(v[f]) for f in abi.SWEEP_VARIANT_FIELDS)


def broken_conditions(row, c, res):
    """What an oracle result of a case lacks of the conditions a case is chosen for, as a list of words (empty: all hold)."""
    n_steps, bad = c["steps"], []
    executed = int(res["steps_executed"].sum())
    if int(res["near_ties"].sum()) != 0:
        bad.append("near ties")
    # (at N = 2 every cell attacks every other: dE = 0 and every move is accepted)
    if not 0 < int(res["n_accepted"].sum()) <= executed or (c["N"] > 2 and int(res["n_accepted"].sum()) == executed):
        bad.append("no accepted or no rejected move")
    stopped = res["hist_len"] < n_steps + 1
    if row[2] and not (stopped.any() and ((~stopped).any() or c["N"] == 2)):  # (N = 2: no chain ever improves, all stop)
        bad.append("no mix of early stops")
    if not row[2] and stopped.any():
        bad.append("a chain stopped early")
    if row[7] and not int(res["n_exchanges"].sum()) > 0:
        bad.append("no exchange")
    return bad


def selecting_sizes(row, c):
    """{N: Q} of the sizes at which case `c` with another N (and, full_3d without schedule sets, Q = N^2 -- None -- or N^2 + 13) selects the row."""
    out = {}
    for N in range(abi.MIN_N, (abi.MAX_N if row[0] else abi.MAX_N_BOARD) + 1):
        other = N * N + 13
        for Q in (None, other) if row[0] and len(c["sched"]) == 1 and other < min(N**3, 32768) else (None,):
            try:
                if N not in out and variant_of(build(dict(c, N=N, Q=Q, init="random", inits=None))[0]) == row:
                    out[N] = Q
            except ValueError:  # a size the library does not take in this form
                pass
    return out
