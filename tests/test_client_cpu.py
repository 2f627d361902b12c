"""The client path (leader directory, routed proposals, tickets) without a GPU:
the record layouts, the new entry points' argument checks, the wrappers' checks
on an unbound engine, and the plain-Python model (tests/client_model.py) over
the oracle on the kind of run the GPU tests compare the kernels against."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import client_model as M
from helpers import abi

ENTRY_POINTS = ["raft_engine_read_leaders", "raft_propose_batch", "raft_propose_batch_dev",
                "raft_engine_resolve_tickets", "raft_engine_resolve_tickets_dev"]

# the model runs: a batch every 5 steps for 300 steps, every ticket resolved each time
BASE = dict(R=5, G=203, seed=11, log_cap=300)
FLAT_REF = dict(BASE, **M.FLAT_MIX)
FLAT_TB = dict(BASE, mode=1, ae_max_entries=4, **M.FLAT_MIX)
RING_TB = dict(BASE, mode=1, ae_max_entries=4, log_window=16, **M.RING_MIX)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(abi.LIB_PATH):
        importlib.import_module("raft-kotlin_amd.build").build()
    return abi.load_library()


def test_record_layouts():
    for ct, dt in ((abi.raft_leader_info, abi.LEADER_DTYPE), (abi.raft_ticket, abi.TICKET_DTYPE),
                   (abi.raft_ticket_state, abi.TICKET_STATE_DTYPE)):
        assert C.sizeof(ct) == 16 and dt.itemsize == 16
        assert [n for n, _ in ct._fields_] == list(dt.names)
        assert [dt.fields[n][1] for n in dt.names] == [0, 4, 8, 12]
    assert set(ENTRY_POINTS) <= set(abi.EXPORTED_SYMBOLS)


def test_entry_points_check_arguments_before_any_device_call(lib):
    g = np.zeros(2, np.int64)
    c = np.zeros(2, np.uint32)
    t = np.zeros(2, abi.TICKET_DTYPE)
    s = np.zeros(2, abi.TICKET_STATE_DTYPE)
    ld = np.zeros(2, abi.LEADER_DTYPE)
    p = lambda a: a.ctypes.data
    assert lib.raft_engine_read_leaders(None, 0, 2, p(ld)) == abi.RAFT_EINVAL
    assert b"null engine" in lib.raft_last_error()
    for fn in (lib.raft_propose_batch, lib.raft_propose_batch_dev):
        assert fn(None, p(g), p(c), p(t), 2) == abi.RAFT_EINVAL
        assert fn(None, None, None, None, 0) == abi.RAFT_EINVAL
    for fn in (lib.raft_engine_resolve_tickets, lib.raft_engine_resolve_tickets_dev):
        assert fn(None, p(g), p(t), p(c), p(s), 2) == abi.RAFT_EINVAL
        assert b"null engine" in lib.raft_last_error()


def _unbound_engine(R=5, cap=8):
    eng = importlib.import_module("raft-kotlin_amd.engine")
    e = object.__new__(eng.RaftEngine)
    e.R, e.cap, e.G, e._h = R, cap, 4, None
    return e


def test_wrappers_reject_bad_arguments_before_any_library_call():
    e = _unbound_engine()
    t3 = np.zeros(3, abi.TICKET_DTYPE)
    with pytest.raises(ValueError):
        e.propose([0, 1, 2], [7, 8])
    with pytest.raises(ValueError):
        e.propose([[0, 1]], [7, 8])
    with pytest.raises(ValueError):
        e.resolve([0, 1, 2], t3[:2], [7, 8, 9])
    with pytest.raises(ValueError):
        e.resolve([0, 1, 2], np.zeros((3, 4), np.int32), [7, 8, 9])      # not ticket records
    with pytest.raises(ValueError):
        e.propose_dev(1024, 2048, 4104, 4)                               # tickets: 16-byte aligned
    with pytest.raises(ValueError):
        e.resolve_dev(1024, 4096, 2048, 8200, 4)
    with pytest.raises(AttributeError):                                  # a good call reaches the (absent) library
        e.propose([0, 1], [7, 8])


def test_model_leaders_and_crafted_batch_reference_mode():
    o, _ = M.crafted_oracle(False)
    ld = M.leaders(o.read_state(), 3)
    assert ld["leader"].tolist() == [-1, 1, 0, 2, 0, 0, 1, -1] and ld["n_leaders"].tolist() == [0, 1, 2, 1, 1, 1, 1, 0]
    assert ld[2].tolist() == (0, 5, 2, 2) and ld[0].tolist() == (-1, 0, 0, 0)
    tk, rc = M.propose(o, M.CRAFTED_GROUPS, M.CRAFTED_CMDS)
    assert rc == abi.RAFT_OK
    assert tk["status"].tolist() == [0, 2, 0, 0, 0, 1, 3, 0, 0, 2, 1, 3]
    assert tk["index"][M.CRAFTED_GROUPS == 1].tolist() == [5, 6, 7]      # consecutive in batch order
    assert tk[6].tolist() == (0, 16, 4, M.LOG_FULL)                      # the crafted LOG_FULL: nothing stored
    st = o.read_state()
    t, c = o.read_log()
    assert st[5, abi.F_INDEX["last"]] == 16 and st[5, abi.F_INDEX["phys"]] == 16
    assert c[1, 1, 5:8].tolist() == M.CRAFTED_CMDS[M.CRAFTED_GROUPS == 1].tolist()
    rec, rrc = M.resolve(st, t, c, M.CRAFTED_GROUPS, tk, M.CRAFTED_CMDS, 3, 16)
    assert rrc == abi.RAFT_OK
    # accepted: pending on the leader alone; ghosted: lost at once; the rest stored nothing
    assert rec["status"].tolist() == [2, 0, 2, 2, 2, 3, 0, 2, 2, 0, 3, 0]
    assert rec["holders"].tolist() == [1, 0, 1, 1, 1, 0, 0, 1, 1, 0, 0, 0] and not rec["committed_on"].any()
    # an entry of group 6's committed prefix, and the same one with another command
    old = np.array([(1, 1, int(t[6, 1, 1]), M.ACCEPTED)] * 2, dtype=abi.TICKET_DTYPE)
    rec, _ = M.resolve(st, t, c, [6, 6], old, [int(c[6, 1, 1]), 5], 3, 16)
    assert rec.tolist() == [(M.COMMITTED, 3, 3, 0), (M.LOST, 0, 0, 0)]
    # a bad group, a bad index, a bad replica: INVALID, the others still filled
    bad = np.array([(1, 5, 4, 0), (1, 16, 4, 0), (3, 5, 4, 0), (1, 5, 4, 0)], dtype=abi.TICKET_DTYPE)
    rec, rrc = M.resolve(st, t, c, [1, 1, 1, 8], bad, [9001] * 4, 3, 16)
    assert rec["status"].tolist() == [M.PENDING, M.INVALID, M.INVALID, M.INVALID] and rrc == abi.RAFT_ERANGE
    rec, rrc = M.resolve(st, t, c, [1, 1, 1], bad[:3], [9001] * 3, 3, 16)
    assert rrc == abi.RAFT_EINVAL
    assert M.propose(o, [0, 8], [1, 2]) == (None, abi.RAFT_ERANGE)


def test_model_crafted_batch_textbook_mode():
    """No ghost tail in an array log: the add lands on slot lastIndex."""
    o, _ = M.crafted_oracle(True)
    tk, rc = M.propose(o, M.CRAFTED_GROUPS, M.CRAFTED_CMDS, textbook=True)
    assert rc == abi.RAFT_OK and tk["status"].tolist() == [0, 2, 0, 0, 0, 0, 3, 0, 0, 2, 0, 3]
    rec, _ = M.resolve(o.read_state(), *o.read_log(), M.CRAFTED_GROUPS, tk, M.CRAFTED_CMDS, 3, 16)
    assert rec["status"].tolist() == [2, 0, 2, 2, 2, 2, 0, 2, 2, 0, 2, 0]


def _statuses(kw, steps=300):
    batches, _, (_, tickets, _), _ = M.oracle_run(steps, 5, **kw)
    return batches, tickets, M.history(batches)


def test_model_reference_mode_sees_every_fate():
    batches, tickets, h = _statuses(FLAT_REF)
    seen = set(tickets["status"].tolist())
    assert seen == {M.ACCEPTED, M.GHOSTED, M.NO_LEADER}, seen            # (LOG_FULL: the crafted case)
    for s in (M.NONE, M.COMMITTED, M.PENDING, M.LOST):
        assert (h == s).any(), s
    assert not (h == M.UNKNOWN).any() and not (h == M.INVALID).any()
    assert all(b["propose_rc"] == abi.RAFT_OK and b["resolve_rc"] == abi.RAFT_OK for b in batches)
    # a ticket that stored nothing stays NONE
    none = (tickets["status"] == M.NO_LEADER)
    assert np.all((h[none] == M.NONE) | (h[none] == -1))


def test_model_textbook_mode_committed_is_final():
    batches, tickets, h = _statuses(FLAT_TB)
    assert not (tickets["status"] == M.GHOSTED).any() and (tickets["status"] == M.ACCEPTED).any()
    assert (h == M.COMMITTED).any() and (h == M.PENDING).any()
    was = np.maximum.accumulate(h == M.COMMITTED, axis=1)                # committed at some earlier resolve
    assert np.all(h[was] == M.COMMITTED)                                 # no ticket ever leaves COMMITTED


def test_model_ring_reports_unknown():
    batches, tickets, h = _statuses(RING_TB)
    assert (h == M.UNKNOWN).any() and (h == M.COMMITTED).any()
    assert any(b["resolve_rc"] == abi.RAFT_EWINDOW for b in batches)
    assert all(b["resolve_rc"] in (abi.RAFT_OK, abi.RAFT_EWINDOW) for b in batches)
