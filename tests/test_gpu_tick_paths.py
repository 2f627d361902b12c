"""The leader tick's rare paths on the engine (marker `gpu`): tail-cache misses
while followers catch up, the loss compares at the drop threshold's edges on
the built-for-the-workload and the general kernel, two sessions in one group
(swap, spill and cancel in one tick), a step-down and the commit replay.

Every scenario (tests/tick_paths_model.py) runs in lockstep with the oracle,
bit-exact on every per-step counter row, the digest after every step, and the
full state and logs at the end; its precondition, checked on the oracle's
trace, shows that the branch it is there for ran."""
import numpy as np
import pytest

import oracle as O
import tick_paths_model as M
from helpers import abi
from test_gpu_parity import RaftEngine, run_lockstep

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(M.SCENARIOS))
def test_tick_path_vs_oracle(name):
    sc = M.SCENARIOS[name]()
    ref = O.Oracle(abi.make_params(**sc["kw"]))                  # the precondition's trace
    M.start(sc, ref)
    sc["check"](M.run_oracle(ref, sc["steps"]))
    e, o = RaftEngine(abi.make_params(**sc["kw"])), O.Oracle(abi.make_params(**sc["kw"]))
    M.start(sc, e, o)
    run_lockstep(e, o, sc["steps"], 1, name)
    assert np.array_equal(o.read_state(), ref.read_state())     # the run the precondition was checked on
    e.close()
