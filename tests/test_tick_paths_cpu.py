"""The tick-path scenarios (tests/tick_paths_model.py) on the oracle alone: every
scenario's precondition -- the rare branch of the leader tick it is there for
really runs -- must hold at the chosen seeds and shapes, so that the GPU
parity test of the same scenarios (tests/test_gpu_tick_paths.py) is not
vacuous."""
import pytest

import oracle as O
import tick_paths_model as M
from helpers import abi


@pytest.mark.parametrize("name", list(M.SCENARIOS))
def test_oracle_produces_the_precondition(name):
    sc = M.SCENARIOS[name]()
    o = O.Oracle(abi.make_params(**sc["kw"]))
    M.start(sc, o)
    sc["check"](M.run_oracle(o, sc["steps"]))
