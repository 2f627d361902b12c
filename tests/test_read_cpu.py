"""Linearizable reads (ReadIndex tickets) without a GPU: the exported names, the
record layouts, the entry points' argument checks, the wrappers' checks on an
unbound engine, the plain-Python model (tests/read_model.py) on hand-built
groups with the expected records written out by hand, and the property -- a
served read reflects every write acknowledged before its begin -- on the oracle
in textbook mode."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import read_model as M
from helpers import abi

ENTRY_POINTS = ["raft_read_begin_batch", "raft_read_begin_batch_dev", "raft_read_serve_batch",
                "raft_read_serve_batch_dev"]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(abi.LIB_PATH):
        importlib.import_module("raft-kotlin_amd.build").build()
    return abi.load_library()


def test_new_names_are_exported(lib):
    assert set(ENTRY_POINTS) <= set(abi.EXPORTED_SYMBOLS)
    for name in ENTRY_POINTS:
        assert getattr(lib, name).restype is C.c_int
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "raft_engine.h")).read()
    import re
    for name, value in [("ISSUED", abi.READ_ISSUED), ("TERM_UNCOMMITTED", abi.READ_TERM_UNCOMMITTED),
                        ("NO_LEADER", abi.READ_NO_LEADER), ("UNKNOWN", abi.READ_UNKNOWN), ("SERVED", abi.READ_SERVED),
                        ("BEHIND", abi.READ_BEHIND), ("GAPPED", abi.READ_GAPPED), ("NO_QUORUM", abi.READ_NO_QUORUM),
                        ("DEPOSED", abi.READ_DEPOSED), ("NONE", abi.READ_NONE), ("INVALID", abi.READ_INVALID)]:
        assert int(re.search(rf"#define RAFT_READ_{name}\s+(\d+)", hdr).group(1)) == value, name
    assert abi.READ_TICKET_STATUS_NAMES[abi.READ_NO_LEADER] == "NO_LEADER"
    assert abi.READ_STATUS_NAMES[abi.READ_DEPOSED] == "DEPOSED" and len(abi.READ_STATUS_NAMES) == 7
    eng = importlib.import_module("raft-kotlin_amd.engine").RaftEngine
    svc = importlib.import_module("raft-kotlin_amd.service").RaftService
    assert callable(eng.begin_reads) and callable(eng.serve_reads) and callable(svc.read_linearizable)


def test_record_layouts():
    for ct, dt in ((abi.raft_read_ticket, abi.READ_TICKET_DTYPE), (abi.raft_read_result, abi.READ_RESULT_DTYPE)):
        assert C.sizeof(ct) == 16 and dt.itemsize == 16
        assert [n for n, _ in ct._fields_] == list(dt.names)
        assert [dt.fields[n][1] for n in dt.names] == [0, 4, 8, 12]


def test_entry_points_check_arguments_before_any_device_call(lib):
    g = np.zeros(2, np.int64)
    k = np.zeros(2, np.uint32)
    t = np.zeros(2, abi.READ_TICKET_DTYPE)
    r = np.zeros(2, abi.READ_RESULT_DTYPE)
    p = lambda a: a.ctypes.data
    for fn in (lib.raft_read_begin_batch, lib.raft_read_begin_batch_dev):
        assert fn(None, p(g), p(t), 2) == abi.RAFT_EINVAL
        assert b"null engine" in lib.raft_last_error()
        assert fn(None, None, None, 0) == abi.RAFT_EINVAL
    for fn in (lib.raft_read_serve_batch, lib.raft_read_serve_batch_dev):
        assert fn(None, p(g), p(t), p(k), p(r), 2) == abi.RAFT_EINVAL
        assert b"null engine" in lib.raft_last_error()
        assert fn(None, None, None, None, None, 0) == abi.RAFT_EINVAL


def _unbound_engine(R=5, cap=8):
    eng = importlib.import_module("raft-kotlin_amd.engine")
    e = object.__new__(eng.RaftEngine)
    e.R, e.cap, e.G, e._h = R, cap, 4, None
    return e


def test_wrappers_reject_bad_arguments_before_any_library_call():
    e = _unbound_engine()
    t3 = np.zeros(3, abi.READ_TICKET_DTYPE)
    with pytest.raises(ValueError):
        e.begin_reads([[0, 1]])
    with pytest.raises(ValueError):
        e.serve_reads([0, 1, 2], t3[:2], [7, 8, 9])
    with pytest.raises(ValueError):
        e.serve_reads([0, 1, 2], t3, [7, 8])
    with pytest.raises(ValueError):
        e.serve_reads([0, 1, 2], np.zeros(3, abi.TICKET_DTYPE), [7, 8, 9])   # a propose ticket is not a read ticket
    with pytest.raises(ValueError):
        e.begin_reads_dev(1024, 4104, 4)                                     # tickets: 16-byte aligned
    with pytest.raises(ValueError):
        e.serve_reads_dev(1024, 4096, 2048, 8200, 4)
    with pytest.raises(AttributeError):                                      # a good call reaches the (absent) library
        e.begin_reads([0, 1])
    svc = importlib.import_module("raft-kotlin_amd.service").RaftService(e)
    with pytest.raises(KeyError):                                            # a key never interned: before any device call
        svc.read_linearizable([0], ["never submitted"])


def test_model_on_the_crafted_groups():
    """One group per status; the expected tickets and records are written out
    by hand in read_model.py (CRAFTED_TICKETS, CRAFTED_RECORDS)."""
    w, t, c, heads, regs = M.crafted()
    R, cap = M.CR, M.CCAP
    tk, rc = M.begin(w, t, M.CRAFTED_GROUPS, R, cap)
    assert rc == abi.RAFT_OK and tk.tolist() == M.CRAFTED_TICKETS.tolist()
    keys = np.full(M.CG, M.KEY + 8 * 5, np.uint32)                           # the key's low bits name the register
    rec, rc = M.serve(w, heads, regs, M.CRAFTED_GROUPS, tk, keys, R, cap)
    assert rec.tolist() == M.CRAFTED_RECORDS.tolist()
    assert rc == abi.RAFT_EINVAL                                             # group 0's NO_LEADER ticket: replica -1
    rec, rc = M.serve(w, heads, regs, M.CRAFTED_GROUPS[1:], tk[1:], keys[1:], R, cap)
    assert rc == abi.RAFT_OK and rec.tolist() == M.CRAFTED_RECORDS[1:].tolist()
    # two leaders of different terms, the stale one at the lower id: begin picks the newer one (ticket 4 above),
    # raft_leader_info.leader the stale one, and a ticket that names the stale one is refused
    import client_model
    assert client_model.leaders(w, R)["leader"][4] == 0 and tk["replica"][4] == 3
    rec, rc = M.serve(w, heads, regs, [4], M.STALE_TICKET, [M.KEY], R, cap)
    assert rc == abi.RAFT_OK and rec.tolist() == M.STALE_RECORD.tolist()
    # BEHIND turns SERVED once the machine has applied the committed prefix
    h2, r2 = heads.copy(), regs.copy()
    h2["applied"][5, 2], r2[5, 2, M.KEY] = 6, c[5, 2, 5]
    rec, _ = M.serve(w, h2, r2, [5], tk[5:6], [M.KEY], R, cap)
    assert rec.tolist() == [(43, M.SERVED, 6, 5)]
    # a restart of the ticket's leader (role FOLLOWER, term kept): DEPOSED
    w2 = w.copy()
    M.set_fld(w2[1:2], R, 2, "role", abi.FOLLOWER)
    rec, _ = M.serve(w2, heads, regs, [1], tk[1:2], [M.KEY], R, cap)
    assert rec.tolist() == [(0, M.DEPOSED, 0, 5)]


def test_model_forged_tickets_and_bad_groups():
    w, t, c, heads, regs = M.crafted()
    R, cap = M.CR, M.CCAP
    good = (2, 3, 6, M.ISSUED)
    forged = np.array([good, (R, 3, 6, M.ISSUED), (-2, 3, 6, M.ISSUED), (2, 3, -1, M.ISSUED), (2, 3, cap + 1, M.ISSUED),
                       (2, 2 ** 31 - 1, 6, M.ISSUED), (2, 3, cap, M.ISSUED), good], dtype=abi.READ_TICKET_DTYPE)
    groups = [1] * len(forged)
    rec, rc = M.serve(w, heads, regs, groups, forged, [M.KEY] * len(forged), R, cap)
    assert rc == abi.RAFT_EINVAL
    assert rec["status"].tolist() == [M.SERVED, M.INVALID, M.INVALID, M.INVALID, M.INVALID, M.DEPOSED, M.BEHIND, M.SERVED]
    assert rec[5].tolist() == (0, M.DEPOSED, 0, 0) and rec[6].tolist() == (0, M.BEHIND, 6, 5)
    for bad in (M.CG, -1):
        groups[3] = bad                                                      # and a bad group: RAFT_ERANGE goes first
        rec, rc = M.serve(w, heads, regs, groups, forged, [M.KEY] * len(forged), R, cap)
        assert rc == abi.RAFT_ERANGE and rec["status"][3] == M.INVALID and rec["status"][7] == M.SERVED
        assert M.begin(w, t, [1, bad, 2], R, cap) == (None, abi.RAFT_ERANGE)


@pytest.mark.parametrize("R", [1, 2])
def test_model_small_groups(R):
    """R = 1: quorum 1, the leader alone confirms itself.  R = 2: quorum 2, so
    one replica a term ahead gives NO_QUORUM."""
    w, t, c, heads, regs = M.small(R)
    tk, rc = M.begin(w, t, [0, 1], R, 4)
    assert rc == abi.RAFT_OK and tk.tolist() == [(0, 2, 1, M.ISSUED)] * 2
    rec, rc = M.serve(w, heads, regs, [0, 1], tk, [77, 77], R, 4)
    assert rc == abi.RAFT_OK
    assert rec.tolist() == [(77, M.SERVED, 1, R), (77, M.SERVED, 1, 1) if R == 1 else (0, M.NO_QUORUM, 0, 1)]


def test_model_ring_slot_below_the_window():
    w, t, c = M.ring()
    tk, rc = M.begin(w, t, [0], 3, 32, W=8)
    assert rc == abi.RAFT_EWINDOW and tk.tolist() == [(1, 2, 3, M.UNKNOWN)]
    tk, rc = M.begin(w, t, [0], 3, 32)                                       # the same state with a flat log
    assert rc == abi.RAFT_OK and tk.tolist() == [(1, 2, 3, M.ISSUED)]
    M.set_fld(w, 3, 1, "commit", 5)                                          # slot 4 is the window's first
    tk, rc = M.begin(w, t, [0], 3, 32, W=8)
    assert rc == abi.RAFT_OK and tk.tolist() == [(1, 2, 5, M.ISSUED)]


def test_property_on_the_oracle_in_textbook_mode():
    """R=5, G=203, seed=11, log_cap=300, textbook, the stress mix; 200 steps in
    rounds of 5: propose to every group, apply on all replicas, begin for every
    group, serve.  The value and ordering assertions are read_model.check_property's.
    From step 100 on (4,060 reads), with the proposals injected, the oracle and
    the models give 2,468 SERVED (61 %), 771 NO_LEADER, 652 TERM_UNCOMMITTED and
    169 NO_QUORUM; the assertions ask for at least half and at least one each."""
    rounds, final = M.property_run(**M.PROPERTY_KW)
    assert len(rounds) == 40 and rounds[-1]["step"] == 195
    n = M.check_property(rounds, final, M.PROPERTY_KW["R"], M.PROPERTY_SLOTS)
    print("reads from step 100 on:", n)
    assert n["reads"] == 20 * 203 == 4060 and n["ISSUED"] > 4000       # (ISSUED: over the whole run, 4,946)
    assert 2 * n["SERVED"] >= n["reads"], n
    assert n["NO_LEADER"] >= 1 and n["TERM_UNCOMMITTED"] >= 1 and n["NO_QUORUM"] >= 1, n
    # the model's serve never meets a malformed ticket here, and a textbook flat log has no window
    assert all(rd["serve_rc"] == abi.RAFT_OK and rd["begin_rc"] == abi.RAFT_OK for rd in rounds)
    assert not any((rd["records"]["status"] == M.GAPPED).any() for rd in rounds)
