"""The step kernel's election bookkeeping on the engine (marker `gpu`): the
cases of tests/election_paths_model.py -- R = 3, 5, 7 at a full, a second and
a partial wave, 300 steps of heavy churn from a crafted start state, drop
thresholds 0, config 3's and 65,536, flat log and two rings, the kernel built
for the workload and the general one, reference and textbook mode -- against
the oracle, bit-exact, at launch lengths 1, 37 and 300.

At one step per launch every counter row and the digest after every step
equal the oracle's, and the full state and logs at the end; the longer
launches give the same counter rows, state, logs and digest.  That holds for
the flat log and for the "ring" layout (the ring kernels with a window of
log_cap slots, where no access can miss).  In the "ringmiss" layout the
log_window (8) is too small for the run on purpose (the window-miss counters
must count): a miss is counted, its value undefined, so the oracle is compared
through the first step that misses (that step's counter row included, the
digest up to the step before it), and from there on the three launch lengths
are compared with each other.  The oracle's runs are computed
once and shared with tests/test_election_paths_cpu.py, which shows that they
reach the paths."""
import numpy as np
import pytest

import election_paths_model as M
from helpers import abi, assert_same_logs, assert_same_state
from test_gpu_parity import RaftEngine

pytestmark = pytest.mark.gpu


def engine_run(kw, general, launch, ref=None):
    """One engine run of the case at `launch` steps per launch: (counter rows,
    state, logs, digest).  With ref (the oracle's run) it steps one launch at
    a time and compares each launch's rows and digest as it goes."""
    e = RaftEngine(abi.make_params(steps_per_launch=launch, kernel=abi.KERNEL_GENERAL if general else abi.KERNEL_AUTO,
                                   **kw))
    try:
        M.start(kw, e)
        if ref is None:
            rows = e.step(M.STEPS)
        else:
            rows, limit = [], ref["first_miss"]
            for t in range(M.STEPS):
                row = e.step(1)
                if t <= limit and not np.array_equal(row[0], ref["rows"][t]):
                    bad = int(np.argwhere(row[0] != ref["rows"][t])[0, 0])
                    raise AssertionError(f"step {t}: {abi.COUNTER_NAMES[bad]} {row[0, bad]} vs the oracle's "
                                         f"{ref['rows'][t, bad]}")
                if t < limit:
                    assert e.digest() == ref["digests"][t], f"digest differs after step {t}"
                rows.append(row[0])
            rows = np.stack(rows)
        return rows, e.read_state(), e.read_log(), e.digest()
    finally:
        e.close()


@pytest.mark.parametrize("case", M.CASES, ids=[M.case_id(c) for c in M.CASES])
def test_election_paths_vs_oracle(case):
    R, layout, mode, drop, general = case
    ref = M.oracle_run(R, layout, mode, drop)
    kw = ref["kw"]
    assert layout == "ringmiss" or ref["first_miss"] == M.STEPS
    rows1, state1, log1, digest1 = engine_run(kw, general, 1, ref)
    if ref["first_miss"] == M.STEPS:                       # no access missed: the whole run is the oracle's
        assert np.array_equal(rows1, ref["rows"])
        assert_same_state(state1, ref["state"], R, M.case_id(case))
        assert_same_logs(state1, log1, ref["log"], R, M.case_id(case))
        assert digest1 == ref["digests"][-1]
    for launch in M.LAUNCHES[1:]:
        rows, state, log, digest = engine_run(kw, general, launch)
        if not np.array_equal(rows, rows1):
            bad = np.argwhere(rows != rows1)[0]
            raise AssertionError(f"launch length {launch}: counters differ from launch length 1 at step {bad[0]} "
                                 f"({abi.COUNTER_NAMES[bad[1]]})")
        assert_same_state(state, state1, R, f"launch length {launch} vs 1")
        assert_same_logs(state1, log, log1, R, f"launch length {launch} vs 1")
        assert digest == digest1, f"launch length {launch}: digest differs from launch length 1"
