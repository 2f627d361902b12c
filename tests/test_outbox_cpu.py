"""The proposal outbox on the oracle alone (no GPU): tests/outbox_model.py, the
reference test_gpu_outbox.py compares the engine's kernels with, checked against
records written out by hand and against the property the outbox exists for.
Every comparison is exact."""
import numpy as np
import pytest

import outbox_model as OM
from helpers import abi


def same(got, want, label=""):
    assert got.dtype == want.dtype and len(got) == len(want), (label, len(got), len(want))
    if not np.array_equal(got, want):
        at = int(np.flatnonzero(got != want)[0])
        raise AssertionError(f"{label}: first difference at {at}: {got[at]} vs {want[at]}")


def test_record_layouts():
    assert abi.OUTBOX_ENTRY_DTYPE.itemsize == 48 and abi.OUTBOX_DONE_DTYPE.itemsize == 32
    import ctypes as C
    assert C.sizeof(abi.raft_outbox_info) == 45 * 8 and abi.RAFT_EFULL == -7


@pytest.mark.parametrize("textbook", [False, True], ids=["reference", "textbook"])
def test_crafted_groups_one_per_verdict(textbook):
    """committed, pending, orphaned (kept, not retried), gone (retried: a new
    ticket, tries 1), no leader, log full, expired, two records of one group
    retried in one pump (consecutive indices): the records written out by hand
    in outbox_model."""
    h = OM.crafted_host(textbook)
    info, done = h.outbox_pump()
    assert info == OM.CRAFTED_INFO and h.last_status == abi.RAFT_OK
    same(done, OM.CRAFTED_DONE, "done")
    same(h.outbox_read(), OM.CRAFTED_LEFT, "queue")
    orphan = h.outbox_read()[3]
    assert orphan["tag"] == 15 and orphan["tries"] == 0 and h.seen_orphaned == {15}
    two = h.outbox_read()[[2, 5]]
    assert two["index"].tolist() == [5, 6] and (two["group"] == 7).all()
    # the oracle took the three accepted adds: the leaders of groups 3 and 7 grew by 1 and 2
    from helpers import fld
    st = h.read_state()
    assert [int(fld(st, OM.CR, 1, "last")[g]) for g in (3, 7, 4, 5)] == [6, 7, 5, OM.CCAP]
    # a second pump with no step in between: nothing is done, the three adds are PENDING, the refused ones retried
    info2, done2 = h.outbox_pump()
    assert len(done2) == 0 and info2["pending"] == 4 and info2["orphaned"] == 1 and info2["retried"] == 2
    assert h.outbox_read()["tries"].tolist() == [1, 2, 1, 0, 2, 1, 2]
    h.close()


@pytest.mark.parametrize("max_done", [0, 1, 2])
def test_the_cut_at_max_done(max_done):
    """A cut at 0, at 1 and in the middle of the three done records: the first
    max_done leave in queue order, the rest count as deferred and stay where
    they were, unchanged; a later pump hands them out."""
    h = OM.crafted_host(True)
    want_done, want_left, want_info = OM.crafted_cut(max_done)
    info, done = h.outbox_pump(max_done)
    assert info == want_info, (info, want_info)
    same(done, want_done, "done")
    same(h.outbox_read(), want_left, "queue")
    info2, rest = h.outbox_pump()
    same(np.concatenate([done, rest]), OM.CRAFTED_DONE, "both pumps")
    assert info2["deferred"] == 0 and info2["committed"] + info2["expired"] == 3 - max_done
    h.close()


def test_below_a_window_is_unknown():
    """A ticket whose slot is below a 16-slot window cannot be judged: kept,
    counted in `unknown`, RAFT_EWINDOW; its neighbour in the window is PENDING."""
    h = OM.Host(**OM.RING_KW)
    w, t, c = OM.crafted_ring()
    h.o.write_state(w)
    h.o.write_log(t, c)
    h.outbox_configure(8)
    h.outbox_write(OM.RING_QUEUE)
    info, done = h.outbox_pump()
    assert info == OM.RING_INFO and h.last_status == abi.RAFT_EWINDOW and len(done) == 0
    same(h.outbox_read(), OM.RING_QUEUE, "queue")
    h.close()


def test_rejections_enqueue_nothing():
    """RAFT_EFULL and RAFT_ERANGE enqueue nothing; configure, reset and
    reconfigure-while-non-empty behave as the header states."""
    h = OM.Host(R=3, G=8, log_cap=16)
    for call in (lambda: h.outbox_submit([0], [1], [1]), lambda: h.outbox_pump(), lambda: h.outbox_read()):
        with pytest.raises(OM.OutboxError) as ei:
            call()
        assert ei.value.code == abi.RAFT_EINVAL                     # not configured
    for bad in ((0, 0), (-1, 0), (4, -1)):
        with pytest.raises(OM.OutboxError):
            h.outbox_configure(*bad)
    h.outbox_configure(4)
    h.outbox_submit([1, 2], [11, 12], [101, 102])
    before = h.outbox_read()
    assert before["status"].tolist() == [OM.NEW] * 2 and before["tries"].tolist() == [0, 0]
    for groups, code in (([1, 2, 3], abi.RAFT_EFULL), ([1, 8], abi.RAFT_ERANGE), ([-1], abi.RAFT_ERANGE)):
        with pytest.raises(OM.OutboxError) as ei:
            h.outbox_submit(groups, [5] * len(groups), [6] * len(groups))
        assert ei.value.code == code
        same(h.outbox_read(), before, "after a refused submit")
    h.outbox_submit([], [], [])                                     # n == 0
    with pytest.raises(OM.OutboxError) as ei:                       # not empty
        h.outbox_configure(8)
    assert ei.value.code == abi.RAFT_EINVAL
    bad = before.copy()
    for field, value, code in (("group", 8, abi.RAFT_ERANGE), ("status", 7, abi.RAFT_EINVAL), ("tries", -1, abi.RAFT_EINVAL)):
        bad[:] = before
        bad[field][1] = value
        with pytest.raises(OM.OutboxError) as ei:
            h.outbox_write(bad)
        assert ei.value.code == code
    bad[:] = before
    bad["status"][0], bad["replica"][0], bad["index"][0] = 0, 3, 2
    with pytest.raises(OM.OutboxError):
        h.outbox_write(bad)
    same(h.outbox_read(), before, "after refused writes")
    h.reset()
    assert h.outbox_len() == 0
    h.outbox_configure(8, 5)                                        # empty: may be configured again
    h.close()


@pytest.mark.parametrize("R,mode,log", OM.PARITY_CASES, ids=[f"R{c[0]}-{c[1]}-{c[2]}" for c in OM.PARITY_CASES])
def test_the_parity_scenario_is_not_vacuous(R, mode, log):
    """What test_gpu_outbox.py compares the engine with: the run completes
    records, defers some at a cut and retries; with more than one replica it
    meets PENDING records as well."""
    tot = OM.totals(OM.host_parity_run(R, mode, log))
    assert tot["committed"] > 0 and tot["retried"] > 0 and tot["deferred"] > 0 and tot["no_leader"] > 0, tot
    assert tot["pending"] > 0 or R == 1, tot


def test_the_parity_scenarios_meet_every_verdict():
    tot = OM.zero_info()
    for case in OM.PARITY_CASES:
        for k, v in OM.totals(OM.host_parity_run(*case)).items():
            if k != "age_hist":
                tot[k] += v
    for k in ("committed", "expired", "deferred", "pending", "orphaned", "unknown", "retried", "accepted", "ghosted",
              "no_leader"):
        assert tot[k] > 0, (k, tot)


def test_commands_commit_once():
    """The property.  Textbook mode, R = 5, G = 203, the stress mix with
    persistent restarts, a submit of distinct commands and a pump every 5
    steps: every COMMITTED completion's (index, term, cmd) lies in the committed
    prefix of a replica's final log; no command occurs under two (index, term)
    in any committed prefix; every submitted tag is completed exactly once or
    still queued."""
    run = OM.property_run(OM.ORPHAN_SEED)
    com = run["completions"]
    assert len(com) > 1000 and (com["status"] == OM.DONE_COMMITTED).all()
    for rec in com:
        g, c = run["cmd_of"][int(rec["tag"])]
        assert g == rec["group"] and (int(rec["index"]), int(rec["term"])) in run["places"][(g, c)], rec
    assert OM.duplicates(run) == []
    tags = com["tag"].tolist() + run["queued"]
    assert len(tags) == len(set(tags)) and set(tags) == set(run["cmd_of"])


def test_an_orphan_commits_later_and_the_naive_rule_commits_it_twice():
    """The case the rule is for, on one input.  Under the outbox's rule at least
    one record is counted `orphaned` (LOST on its own replica, held by another)
    and later completes COMMITTED, and no command is committed twice.  The naive
    rule (retry every LOST), run in the model on the same input, commits a
    command under two (index, term)."""
    run = OM.property_run(OM.ORPHAN_SEED)
    com = run["completions"]
    late = [t for t in com["tag"][com["status"] == OM.DONE_COMMITTED].tolist() if t in run["orphaned"]]
    assert len(late) >= 1 and run["totals"]["orphaned"] >= 1
    assert OM.duplicates(run) == []
    naive = OM.property_run(OM.ORPHAN_SEED, "naive")
    twice = OM.duplicates(naive)
    assert len(twice) >= 1, "the naive rule committed nothing twice on this input"
    assert all(len(naive["places"][k]) >= 2 for k in twice)
