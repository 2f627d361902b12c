"""The election-path cases (tests/election_paths_model.py) on the oracle alone:
every case must reach the paths the step kernel's election bookkeeping
distinguishes, at the chosen seeds and shapes, so that the GPU parity test of
the same cases (tests/test_gpu_election_paths.py) is not vacuous.  The
conditions are on the oracle's own states and counter rows.

With a working network (drop thresholds 0 and config 3's) a case reaches all
of them: a timer firing while the replica is already electing, two
RequestVote senders of one group in one step, a backoff ending in a restart
and one ending the election, an election ending with a queued follower reset,
a heartbeat session cancelled as stale, a session started in D and ticked in
the same step (its group replayed alone: its own tick count), and
LOG_OVERFLOW > 0 -- each at a step the GPU test compares with the oracle, that
is, no later than the first step with a window miss.  Only the "ringmiss"
layout misses (at about step 12, before its log_cap can overflow): it is there
for LOG_WINDOW_MISS > 0, which it must reach, and the "ring" layout of the same
kernels reaches every other path with the whole run compared.  With every
message lost (threshold 65,536) nobody is ever elected, so that case reaches
the election-loop paths only; its family reaches the rest through its other
two cases."""
import pytest

import election_paths_model as M


@pytest.mark.parametrize("fam", M.FAMILIES, ids=[M.family_id(f) for f in M.FAMILIES])
def test_oracle_reaches_every_path(fam):
    layout = fam[1]
    for drop in M.DROPS:
        run = M.oracle_run(*fam, drop)
        compared = run["first_miss"]                       # the last step compared with the oracle
        if drop == "dropall":
            need = M.ELECTION_PATHS
        elif layout == "ringmiss":
            need = ("log_window_miss",)
        else:
            need = M.ALL_PATHS
        missing = [p for p in need if not [t for t in run["hits"].get(p, []) if t <= compared]]
        assert not missing, f"{M.family_id(fam)} {drop}: the oracle never takes {missing} in the compared steps"
        # most steps have an electing group: a vote round starts or a vote is granted
        rows = run["rows"]
        busy = int(((rows[:, M.C["rounds"]] > 0) | (rows[:, M.C["votes_granted"]] > 0)).sum())
        assert busy > M.STEPS // 2, f"{M.family_id(fam)} {drop}: only {busy} steps with an election"
        if layout != "ringmiss" or drop == "dropall":
            assert run["first_miss"] == M.STEPS


def test_shapes_cover_a_full_a_second_and_a_partial_wave():
    for R in (3, 5, 7):
        gpw = 64 // R
        assert M.groups_of(R) == 2 * gpw + 1 and 0 < M.groups_of(R) * R - 2 * gpw * R < 64
