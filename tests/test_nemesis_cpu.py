"""Scripted network faults on the oracle (no GPU): tests/nemesis_model.py's
isolate / heal / list driven through read_state -> model -> write_state, and
what the other side paths promise about a leader cut off from its group, seen
on purpose instead of waiting for the churn harness."""
import functools

import numpy as np
import pytest

import audit_model as AM
import nemesis_model as NM
import outbox_model as OM
import read_model as RD
import sm_model as SM
from helpers import abi, fld
from read_model import newest_leader

# Textbook mode, five replicas, no random fault at all.  The reference's timers
# (an election timeout of 20..23 s under a 2 s step) make most elections tie, and
# without drops to break the ties a group can stay leaderless for hundreds of
# steps; these spread the timeouts over 5..30 steps of 1 s, so the step counts
# below are short.  Found by running the oracle: every group has a leader after
# 20 steps (70 are run); after its leader is cut off the slowest group has a new
# one 23 steps later (59 are run); a healed stale leader is a follower of the new
# term after 1 step (5 are run).
LEADER_KW = dict(R=5, G=24, seed=11, log_cap=300, mode=abi.MODE_TEXTBOOK, ae_max_entries=4, cmd_ppm=250_000,
                 heartbeat_ms=1000, election_min_ms=5000, election_max_ms=30000, backoff_min_ms=1000,
                 backoff_max_ms=10000, round_timeout_ms=3000, retry_ms=2000)
WARMUP, ISOLATE_STEPS, AFTER_HEAL, SLOTS, KEY = 70, 60, 5, 4, 1
# The same scenario under the reference's own timers, lengthened instead: found by running the oracle, the last
# group has its first leader after 1040 steps (1100 are run), the slowest group replaces a cut-off leader after
# 3166 steps (3999 are run), a healed stale leader is a follower of the new term after 1 step (5 are run).  A
# command every 20th group-step keeps the logs inside log_cap; the ledger is observed every 10th step.
DEFAULT_KW = dict(R=5, G=24, seed=11, log_cap=512, mode=abi.MODE_TEXTBOOK, ae_max_entries=4, cmd_ppm=50_000)
# name -> (raft_params, warm-up, steps of the isolation, steps after heal, observe the ledger every)
RUNS = {"fast": (LEADER_KW, WARMUP, ISOLATE_STEPS, AFTER_HEAL, 1), "default": (DEFAULT_KW, 1100, 4000, 5, 10)}
R, G = LEADER_KW["R"], LEADER_KW["G"]
ALL = np.arange(G, dtype=np.int64)


def col(state, name: str, reps) -> np.ndarray:
    """Field `name` of replica reps[g] of every group g."""
    return np.array([int(fld(state, R, int(reps[g]), name)[g]) for g in range(G)])


def newest(state) -> np.ndarray:
    return np.array([newest_leader(state, R, g) for g in range(G)])


@functools.lru_cache(maxsize=None)
def leader_run(name: str = "fast") -> dict:
    """Warm up, isolate every group's newest leader, run the isolation out to
    its last cut step, heal, run on (RUNS[name]).  An audit ledger is observed
    along the way.  Read-only for the tests."""
    kw, warmup, iso_steps, after_heal, every = RUNS[name]
    h = NM.Host(SLOTS, **kw)
    out = dict(flagged=[], commit=[], remaining=[], listed=[], steps=(warmup, iso_steps, after_heal))

    def step():
        h.step(1)
        if h.step_index % every == 0:
            out["flagged"].append(h.observe()["flagged"])

    for _ in range(warmup):
        step()
    st = h.read_state()
    old = newest(st)
    out.update(old=old, old_term=col(st, "term", np.maximum(old, 0)), commit0=col(st, "commit", np.maximum(old, 0)))
    # a ReadIndex ticket on the leader about to be cut off
    h.sm_apply()
    out["early_tickets"], _ = RD.begin(st, h.read_log()[0], ALL, R, h.cap)
    out["tickets"] = h.isolate(ALL, NM.NEWEST, iso_steps)
    for s in range(1, iso_steps):                                    # the word cuts steps - 1 steps
        step()
        st = h.read_state()
        info, rec = h.isolated()
        out["commit"].append(col(st, "commit", old))
        out["remaining"].append(rec["remaining"].copy())
        out["listed"].append((info, rec["group"].copy(), rec["replica"].copy(), rec["role"].copy()))
    out["cut_state"] = st = h.read_state()
    # the reads, while the deposed leader still calls itself LEADER
    h.sm_apply()
    groups, keys = ALL.tolist(), [KEY] * G
    out["plain"] = SM.get(st, h.mach, R, groups, keys, [-1] * G)
    out["begin"], _ = RD.begin(st, h.read_log()[0], ALL, R, h.cap)
    out["serve_early"], _ = RD.serve(st, *h.sm_read(), ALL, out["early_tickets"], keys, R, h.cap)
    out["heal"] = h.heal_network()
    out["healed_words"] = h.read_state()[:, NM.ISO].copy()
    for _ in range(after_heal):
        step()
    out["flagged"].append(h.observe()["flagged"])
    out["end_state"] = h.read_state()
    out["after"] = h.isolated()
    h.close()
    return out


@pytest.mark.parametrize("name", list(RUNS))
def test_an_isolated_leader_is_deposed_and_steps_down_after_heal(name):
    """Under timers that make the run short, and under the reference's own with the run lengthened."""
    run = leader_run(name)
    old = run["old"]
    assert (old >= 0).all(), "the warm-up leaves a group without a leader"
    assert run["tickets"].tolist() == [(int(r), run["steps"][1], NM.SET, 0) for r in old]
    # while it runs the isolated replica's commitIndex does not advance, in any group at any step
    for s, c in enumerate(run["commit"], 1):
        assert np.array_equal(c, run["commit0"]), (s, c, run["commit0"])
    # before it ends every group has a LEADER of a higher term among the other four; the old one still says LEADER
    st = run["cut_state"]
    new = newest(st)
    assert (new >= 0).all() and (new != old).all(), (new, old)
    assert (col(st, "term", new) > run["old_term"]).all()
    assert (col(st, "role", old) == abi.LEADER).all() and np.array_equal(col(st, "term", old), run["old_term"])
    # after heal plus a few steps it is a FOLLOWER of the new term
    assert run["heal"] == dict(healed=G, idle=0, kept=0) and (run["healed_words"] == 0).all()
    end = run["end_state"]
    lead = newest(end)
    assert (lead >= 0).all() and (col(end, "role", old) == abi.FOLLOWER).all()
    assert np.array_equal(col(end, "term", old), col(end, "term", lead))
    assert (col(end, "term", old) > run["old_term"]).all()
    assert run["after"][0] == dict(delivered=0, pending=0, running=0) and len(run["after"][1]) == 0
    # the ledger stays clean throughout
    total = run["steps"][0] + run["steps"][1] - 1 + run["steps"][2]
    assert run["flagged"] == [0] * len(run["flagged"]) and len(run["flagged"]) == total // RUNS[name][4] + 1


def test_remaining_counts_down_by_one_per_step():
    run = leader_run()
    for s, (rem, (info, groups, reps, roles)) in enumerate(zip(run["remaining"], run["listed"]), 1):
        assert info == dict(delivered=G, pending=0, running=G)
        assert (rem == ISOLATE_STEPS - s).all() and np.array_equal(groups, ALL) and np.array_equal(reps, run["old"])
        assert (roles == abi.LEADER).all()
    assert run["remaining"][-1].tolist() == [1] * G                  # the next step's decrement ends it


def test_the_stale_leader_read():
    """The plain leader-routed read answers from the lowest-id LEADER: in the
    groups where the deposed leader has the lower index that is the deposed
    one.  The ReadIndex pair does not: begin names the new leader, and a ticket
    taken on the old leader before the cut is refused (it cannot find a
    quorum in its term)."""
    run = leader_run()
    st, old = run["cut_state"], run["old"]
    new = newest(st)
    shadowed = old < new
    assert shadowed.sum() >= 1 and (~shadowed).sum() >= 1, "both orders of (deposed, new) are needed"
    assert np.array_equal(run["plain"]["replica"][shadowed], old[shadowed])
    assert np.array_equal(run["plain"]["replica"][~shadowed], new[~shadowed])
    assert np.array_equal(run["begin"]["replica"], new) and (run["begin"]["replica"] != old).all()
    early = run["early_tickets"]
    assert np.array_equal(early["replica"], old)
    issued = early["status"] == RD.ISSUED
    assert issued.sum() >= 1
    assert (run["serve_early"]["status"][issued] == RD.NO_QUORUM).all()
    assert (run["serve_early"]["agree"][issued] == 1).all()


class OutboxHost(NM.Calls, OM.Host):
    """outbox_model's Host with the three calls."""


def test_an_outbox_record_on_an_isolated_leader_commits_once():
    """Submit, pump once (the leader appends), isolate the leader before the
    entry replicates.  While the cut lasts the record is kept, PENDING or
    orphaned, and never retried; after heal the old leader's log is overwritten,
    the record is retried, and every command is committed under exactly one
    (index, term)."""
    h = OutboxHost(**LEADER_KW)
    h.step(WARMUP)
    h.outbox_configure(64, 0)
    cmds = (1000 + np.arange(G)).astype(np.uint32)
    h.outbox_submit(ALL, cmds, cmds.astype(np.int64))
    info, done = h.outbox_pump()
    assert info["accepted"] == G and len(done) == 0
    old = h.outbox_read()["replica"].copy()
    assert np.array_equal(old, newest(h.read_state()))
    assert (h.isolate(ALL, NM.NEWEST, ISOLATE_STEPS)["status"] == NM.SET).all()
    completions = []
    for s in range(1, ISOLATE_STEPS):
        h.step(1)
        if s % 5 == 0:
            info, done = h.outbox_pump()
            assert len(done) == 0 and info["retried"] == 0 and info["pending"] + info["orphaned"] == G, (s, info)
    assert h.heal_network()["healed"] == G
    retried = 0
    for _ in range(12):
        h.step(5)
        info, done = h.outbox_pump()
        retried += info["retried"]
        completions.append(done)
        if info["left"] == 0:
            break
    done = np.concatenate(completions)
    assert info["left"] == 0 and retried >= 1
    assert sorted(done["tag"].tolist()) == cmds.tolist() and (done["status"] == OM.DONE_COMMITTED).all()
    places = OM.committed_places(h.read_state(), *h.read_log(), R, h.cap)
    for g, c in zip(ALL.tolist(), cmds.tolist()):
        assert len(places.get((g, c), ())) == 1, (g, c, places.get((g, c)))
    h.close()


def test_crafted_statuses():
    """SET by index and by both leader selectors, NO_LEADER, BUSY (a running
    word, one with a single step left included), the four ways to be INVALID;
    REPLACE turns BUSY into SET.  The tickets are written out by hand."""
    w, tgt, stp, want, forced = NM.crafted()
    n = len(NM.CRAFTED_NAMES)
    for replace, exp in ((False, want), (True, forced)):
        st = w.copy()
        tk, rc = NM.isolate(st, np.arange(n), tgt, stp, NM.CR, replace)
        assert rc == abi.RAFT_OK and tk.tolist() == exp.tolist()
        changed = np.argwhere(st != w)
        sets = np.nonzero(exp["status"] == NM.SET)[0]
        assert changed[:, 0].tolist() == sets.tolist() and (changed[:, 1] == w.shape[1] + NM.ISO).all()
        assert st[sets, NM.ISO].tolist() == [9 << 8 | int(r) for r in exp["replica"][sets]]
    st = w.copy()
    assert NM.isolate(st, [0, n], 0, 5, NM.CR) == (None, abi.RAFT_ERANGE) and np.array_equal(st, w)
    assert NM.isolate(st, [-1], 0, 5, NM.CR) == (None, abi.RAFT_ERANGE)


def test_three_messages_to_one_group():
    """Positions 5, 2 and 9 of a batch of ten name group 3: 2 is judged, the
    others answer DUPLICATE with 2; an INVALID message before them takes no part."""
    w, *_ = NM.crafted()
    groups = np.array([0, 3, 3, 1, 2, 3, 4, 5, 6, 3], dtype=np.int64)
    targets = np.array([0, NM.CR, 2, 0, 0, 4, 0, 0, 0, 1], dtype=np.int32)   # position 1: INVALID, to the same group
    steps = np.array([5, 5, 6, 5, 5, 7, 5, 5, 5, 8], dtype=np.int32)
    st = w.copy()
    tk, rc = NM.isolate(st, groups, targets, steps, NM.CR)
    assert rc == abi.RAFT_OK
    assert tk[[1, 2, 5, 9]].tolist() == [(-1, 5, NM.INVALID, 0), (2, 6, NM.SET, 0), (-1, 7, NM.DUPLICATE, 2),
                                         (-1, 8, NM.DUPLICATE, 2)]
    assert st[3, NM.ISO] == 6 << 8 | 2
    # the same messages in reversed order: the winner is the lowest position of THAT batch
    st = w.copy()
    tk, _ = NM.isolate(st, groups[::-1], targets[::-1], steps[::-1], NM.CR)
    assert tk[[0, 4, 7, 8]].tolist() == [(1, 8, NM.SET, 0), (-1, 7, NM.DUPLICATE, 0), (-1, 6, NM.DUPLICATE, 0),
                                         (-1, 5, NM.INVALID, 0)]
    assert st[3, NM.ISO] == 8 << 8 | 1


def test_heal_with_a_mask_and_the_listing_cut():
    w, *_ = NM.crafted()
    n = w.shape[0]
    st = w.copy()
    NM.isolate(st, np.arange(n), np.arange(n) % NM.CR, 9, NM.CR, replace=True)
    full_info, full = NM.list_isolated(st, NM.CR)
    k = len(full)
    assert k == n and full_info == dict(delivered=k, pending=0, running=k)
    assert full["group"].tolist() == list(range(n)) and full["replica"].tolist() == [g % NM.CR for g in range(n)]
    assert (full["remaining"] == 9).all()
    # cut at max_events: the pieces of successive ranges concatenate to the uncut list
    for room in (0, 1, k - 1, k):
        info, rec = NM.list_isolated(st, NM.CR, max_events=room)
        assert info == dict(delivered=room, pending=k - room, running=k) and rec.tolist() == full[:room].tolist()
        if 0 < room < k:
            g_next = int(rec["group"][-1]) + 1
            _, rest = NM.list_isolated(st, NM.CR, g0=g_next, n=n - g_next)
            assert np.concatenate([rec, rest]).tolist() == full.tolist()
    # heal replicas 0 and 2 only
    mask = np.full(n, 0b00101, np.uint8)
    info = NM.heal(st, NM.CR, mask)
    sel = np.isin(np.arange(n) % NM.CR, (0, 2))
    assert info == dict(healed=int(sel.sum()), idle=0, kept=int((~sel).sum()))
    assert (st[sel, NM.ISO] == 0).all() and (st[~sel, NM.ISO] != 0).all()
    assert NM.heal(st, NM.CR) == dict(healed=int((~sel).sum()), idle=int(sel.sum()), kept=0)
    assert (st[:, NM.ISO] == 0).all() and NM.list_isolated(st, NM.CR)[0] == dict(delivered=0, pending=0, running=0)


def test_record_layouts():
    import ctypes as C
    assert abi.ISOLATE_TICKET_DTYPE.itemsize == C.sizeof(abi.raft_isolate_ticket) == 16
    assert abi.ISOLATED_DTYPE.itemsize == C.sizeof(abi.raft_isolated) == 16
    assert C.sizeof(abi.raft_heal_info) == C.sizeof(abi.raft_isolated_info) == 32
