"""Snapshot install on the oracle alone (no GPU): the inputs of
test_gpu_snapshot.py are not vacuous.  The install is tests/snapshot_model.py's
numpy restatement applied through read_state -> model -> write_state /
write_log; what is asserted here is that the scenarios the engine is compared
against meet every case of the definition."""
import numpy as np
import pytest

import restart_model as RM
import sm_model as M
import snapshot_model as SM
from helpers import F, abi, fld, log_matching_flags

NF = abi.NUM_FIELDS


def total_hits(variant):
    tot = dict.fromkeys(SM.HIT_KEYS, 0)
    for R, G, v in RM.PARITY_CASES:
        if v == variant:
            for k, n in SM.host_parity_run(R, G, v)[1].items():
                tot[k] += n
    return tot


@pytest.mark.parametrize("variant", ["flat", "ring", "textbook"])
def test_parity_scenario_meets_every_case(variant):
    """Over restart_model.PARITY_SHAPES the two installs of the parity scenario
    meet: replicas with a shorter and with an equal-length log, replicas skipped
    as ahead and for lag, groups without a leader, groups with one LEADER (it
    owns the primary session slot once it has ticked) and with two (the slot
    alternates between them), on a ring leaders with physLen below and at or
    above W, on a flat log installs of more than 64 slots.
    An installed ex-leader is not among them: a deposed leader keeps taking
    commands while it is cut off, so in every two-leader group the stress mix
    produced its log was longer than its successor's (lastIndex_L - lastIndex_f
    < 0: skipped for lag); test_installed_ex_leader builds one."""
    h = total_hits(variant)
    print(variant, h)
    for k in ("shorter", "equal", "ahead", "lag_skipped", "no_leader", "one_leader", "two_leaders"):
        assert h[k] > 0, (variant, k, h)
    if variant == "ring":
        assert h["ring_short"] > 0 and h["ring_full"] > 0, h
    else:
        assert h["flat_over_64"] > 0, h


def test_parity_scenario_infos():
    """The infos count what the hits count, the masked install skips groups (its
    range is [3, G - 2)) and the n == 0 call (R = 1, G = 5) is all zeros."""
    pts, hits, _ = SM.host_parity_run(5, 203, "flat")
    infos = [p["info"] for p in pts if "installed" in p.get("info", {})]
    assert len(infos) == 2 and all(set(i) == set(SM.INFO_KEYS) for i in infos)
    assert sum(i["installed"] for i in infos) == hits["shorter"] + hits["equal"] > 0
    assert sum(i["ahead"] for i in infos) == hits["ahead"] and sum(i["no_leader"] for i in infos) == hits["no_leader"]
    assert infos[0]["slots_copied"] > 64 * 5
    pts, _, _ = SM.host_parity_run(1, 5, "flat")
    assert all(not any(p["info"].values()) for p in pts if "installed" in p.get("info", {}))


def test_installed_ex_leader():
    """A deposed leader (role LEADER, a lower term) with a shorter log is
    installed like any follower: FOLLOWER at the leader's term, its vote
    forgotten, its session rows zero, the leader's session towards it caught up."""
    h = SM.Host(RM.PARITY_SLOTS, **SM.EX_LEADER_KW)
    g, L, f = SM.craft_ex_leader(h)
    before = h.read_state()
    info = h.install_snapshot(np.array([1 << f], np.uint8), g0=g)
    after, (t, c) = h.read_state(), h.read_log()
    h.close()
    R = h.R
    assert info == dict(installed=1, slots_copied=int(fld(before, R, L, "phys")[g]), no_leader=0, leader_gapped=0,
                        ahead=0) and h.ihits["ex_leader"] == 1
    for name in ("term", "last", "phys"):
        assert fld(after, R, f, name)[g] == fld(before, R, L, name)[g]
    assert fld(after, R, f, "role")[g] == abi.FOLLOWER and fld(after, R, f, "voted")[g] == -1
    assert fld(after, R, f, "flags")[g] == abi.FL_ARMED
    assert not after[g, R * NF + f * R:R * NF + (f + 1) * R].any()
    assert after[g, R * NF + L * R + f] == fld(before, R, L, "last")[g] + 1
    assert after[g, R * NF + R * R + L * R + f] == fld(before, R, L, "last")[g]
    assert np.array_equal(t[g, f], t[g, L]) and np.array_equal(c[g, f], c[g, L])
    keep = np.ones(before.shape, bool)
    keep[g] = False
    assert np.array_equal(after[keep], before[keep])


def test_ring_stays_valid_on_the_oracle():
    """The validity scenario (snapshot_model.VALID_KW): without the install the
    oracle counts window misses; with RaftService.heal's calls it counts none,
    no dual leader, no log mismatch, no diverged machine and no machine lost an
    entry, while replicas were in fact installed on wrapped rings."""
    a, _, _ = SM.host_validity_run(False)
    assert a["counters"][:, abi.C_INDEX["log_window_miss"]].sum() > 0
    b, hits, mach = SM.host_validity_run(True)
    c = b["counters"]
    assert hits["ring_full"] > 100 and hits["shorter"] > 100, hits
    assert c[:, abi.C_INDEX["commits"]].sum() > 0 and c[:, abi.C_INDEX["log_overflow"]].sum() == 0
    per_40 = c[SM.VALID_WARM:SM.VALID_WARM + 40, abi.C_INDEX["commands"]].sum() / SM.VALID_KW["G"]
    assert per_40 > 16, per_40                                        # a leader appends more than W entries in 40 steps
    assert c[:, abi.C_INDEX["log_window_miss"]].sum() == 0
    assert c[:, abi.C_INDEX["dual_leader_groups"]].sum() == 0
    assert log_matching_flags(b["state"], *b["logs"], SM.VALID_KW["R"], SM.VALID_KW["log_window"]).sum() == 0
    assert M.check(mach).sum() == 0
    assert not (mach.lost != 0).any()
