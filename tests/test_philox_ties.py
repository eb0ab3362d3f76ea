"""GPU: every sweep kernel of the Philox stream -- the 26 plain rows of SWEEP_TABLE with PHILOX and the 7 under replica exchange -- on beta
tables crafted to put the uniform next to exp (near_tie_util.PHILOX_CASES, exchange_tie_util.PHILOX_CASES; the oracle's side, the word count
the crafting rests on and the rows the cases select are pinned on the CPU by tests/test_philox_ties_host.py).  Each case runs bracketed and
with MCQ_FLAG_EXACT_EXP, and both runs are the oracle's bit for bit: every field of util.RESULT_FIELDS, histories and accept bits or the
reduced sums, near_ties per chain (a nonzero total, the crafted one), under exchange exchange_rung and n_exchanges, and each crafted accept
bit.  tests/test_philox.py holds the same kernels to the oracle only where near_ties is 0.  A Philox run cannot be resumed, so there is no
test in segments.

ASSUMPTION of the tie points, as in tests/test_near_ties.py: the device's float64 exp and glibc's agree within 1 ulp at the crafted
arguments (x in [0.05, 1]).  A Philox case that differs at a crafted point while the MT19937 case of its shape passes is a fault of the
Philox path; one that differs in the exact-exp run too, at an argument no MT19937 case holds, is first a measurement of exp
(profiles/near_ties.md)."""
import pytest

from tests import exchange_tie_util as xt
from tests import near_tie_util as nt
from tests import test_exchange_ties as gpu_x
from tests import test_near_ties as gpu

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", [c.name for c in nt.PHILOX_CASES])
def test_philox_sweep_equals_the_oracle_next_to_exp(name):
    assert nt.CASES_BY_NAME[name].rng == "philox"
    gpu.sweep_equals_the_oracle_next_to_exp(name, row=nt.PHILOX_ROW[name])


@pytest.mark.parametrize("name", [c.name for c in xt.PHILOX_CASES])
def test_philox_exchange_equals_the_oracle_next_to_exp(name):
    assert xt.CASES_BY_NAME[name].rng == "philox"
    gpu_x.exchange_equals_the_oracle_next_to_exp(name, row=xt.PHILOX_ROW[name])
