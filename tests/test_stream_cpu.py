"""The binding's record-stream helper (engine._RecordStream) against a fake C
function: what the six streams -- drain_committed, poll_leaders, isolated,
the audit's and the monitor's report, the persistence stream's poll -- and
their _dev twins share, without a GPU."""
import ctypes as C
import importlib
import types

import numpy as np
import pytest

from helpers import abi

eng = importlib.import_module("raft-kotlin_amd.engine")


class FakeEntry:
    """An entry point of the shape (h, g0, n, [selectors,] out, room, &info)
    with `have` records to hand out: it fills delivered and pending, writes
    record j with group g0 + j into the buffer it is given, logs (out, room)
    and returns `rc`."""

    def __init__(self, have: int, dtype, rc: int = abi.RAFT_OK):
        self.have, self.dtype, self.rc, self.calls, self.log = have, dtype, rc, [], []

    def __call__(self, h, g0, n, *rest):
        out, room, info = rest[-3:]
        self.calls.append((out.value, room))
        self.log.append("call")
        k = min(room, self.have) if out.value else 0
        if k:
            raw = (C.c_byte * (k * self.dtype.itemsize)).from_address(out.value)
            np.frombuffer(raw, dtype=self.dtype)["group"] = g0 + np.arange(k)
        info._obj.delivered, info._obj.pending = k, self.have - k
        return self.rc


def engine_with(**entries):
    """A RaftEngine shell over fake entry points (no library, no device)."""
    e = object.__new__(eng.RaftEngine)
    e.R, e.G, e._h = 3, 8, C.c_void_p(7)
    e._lib = types.SimpleNamespace(raft_last_error=lambda: b"boom", **entries)
    return e


def test_no_room_given_peeks_then_fetches():
    f = FakeEntry(5, abi.EVENT_DTYPE)
    info, ev = engine_with(raft_engine_poll_leaders=f).poll_leaders(g0=2)
    assert [c[1] for c in f.calls] == [0, 5] and f.calls[0][0] is None and f.calls[1][0]
    assert ev.dtype == abi.EVENT_DTYPE and ev["group"].tolist() == [2, 3, 4, 5, 6]
    assert info == dict(delivered=5, pending=0, gained=0, lost=0, moved=0, reterm=0, leaderless=0)


@pytest.mark.parametrize("room", [0, 1, 3, 9, np.int64(3)])
def test_a_room_makes_one_call_and_never_a_null_buffer(room):
    f = FakeEntry(5, abi.EVENT_DTYPE)
    info, ev = engine_with(raft_engine_poll_leaders=f).poll_leaders(max_events=room)
    assert len(f.calls) == 1 and f.calls[0][0] and f.calls[0][1] == int(room)
    k = min(int(room), 5)
    assert len(ev) == k == info["delivered"] and info["pending"] == 5 - k        # sliced to delivered
    assert ev["group"].tolist() == list(range(k))
    assert "status" not in info


def test_peek_is_one_null_call_and_an_empty_array_of_the_dtype():
    for name, method, dtype in (("raft_engine_poll_leaders", "poll_leaders", abi.EVENT_DTYPE),
                                ("raft_engine_list_isolated", "isolated", abi.ISOLATED_DTYPE)):
        f = FakeEntry(5, dtype)
        info, rec = getattr(engine_with(**{name: f}), method)(peek=True)
        assert f.calls == [(None, 0)] and info["pending"] == 5 and info["delivered"] == 0
        assert rec.shape == (0,) and rec.dtype == dtype


def test_a_survivable_code_is_the_status_and_any_other_raises():
    f = FakeEntry(4, abi.APPLIED_DTYPE, rc=abi.RAFT_EWINDOW)
    rec, info = engine_with(raft_engine_drain_committed=f).drain_committed()     # (records, info) for the drain
    assert len(rec) == 4 and info["status"] == abi.RAFT_EWINDOW and [c[1] for c in f.calls] == [0, 4]
    f = FakeEntry(4, abi.APPLIED_DTYPE)
    e = engine_with(raft_engine_drain_committed=f)
    assert e.drain_committed(max_entries=2)[1] == dict(delivered=2, pending=2, lost=0, regressed=0, status=abi.RAFT_OK)
    assert e.peek_committed()["pending"] == 4 and f.calls[-1] == (None, 0)
    for rc in (abi.RAFT_ERANGE, abi.RAFT_EINVAL):
        with pytest.raises(eng.RaftError, match="boom"):
            engine_with(raft_engine_drain_committed=FakeEntry(4, abi.APPLIED_DTYPE, rc=rc)).drain_committed()
    # the watch survives no code: RAFT_EWINDOW raises there
    with pytest.raises(eng.RaftError, match="poll_leaders failed"):
        engine_with(raft_engine_poll_leaders=FakeEntry(1, abi.EVENT_DTYPE, rc=abi.RAFT_EWINDOW)).poll_leaders()


def test_a_bad_room_is_refused_before_any_call():
    f = FakeEntry(5, abi.APPLIED_DTYPE)
    e = engine_with(raft_engine_drain_committed=f, raft_engine_drain_committed_dev=f)
    for bad in (-1, True, 2.0, "3"):
        with pytest.raises(ValueError, match="drain_committed: max_entries must be None or an integer >= 0"):
            e.drain_committed(max_entries=bad)
        with pytest.raises(ValueError, match="drain_committed_dev: max_entries"):
            e.drain_committed_dev(0x1000, bad)
    assert f.calls == []


def test_dev_refuses_bad_buffers_before_any_call_and_then_waits_and_calls_once():
    f = FakeEntry(5, abi.EVENT_DTYPE)
    e = engine_with(raft_engine_poll_leaders_dev=f,
                    raft_engine_wait_stream=lambda h, s: f.log.append(("wait", s.value)) or abi.RAFT_OK)
    with pytest.raises(ValueError, match="poll_leaders_dev: a device buffer and its max_events are required"):
        e.poll_leaders_dev(0, 4)                                   # null with room > 0
    with pytest.raises(ValueError, match="required"):
        e.poll_leaders_dev(0x1000, None)
    with pytest.raises(ValueError, match="poll_leaders_dev: the record buffer must be 8-byte aligned"):
        e.poll_leaders_dev(0x1004, 4)
    for bad in (-1, True):
        with pytest.raises(ValueError, match="max_events"):
            e.poll_leaders_dev(0x1000, bad, after_stream=5)
    assert f.calls == [] and f.log == []
    buf = np.zeros(4, dtype=abi.EVENT_DTYPE)                       # stands in for device memory
    info = e.poll_leaders_dev(buf.ctypes.data, 4, g0=1, after_stream=5)
    assert f.log == [("wait", 5), "call"] and f.calls == [(buf.ctypes.data, 4)]
    assert info["delivered"] == 4 and info["pending"] == 1 and buf["group"].tolist() == [1, 2, 3, 4]
    assert e.poll_leaders_dev(0, 0)["delivered"] == 0              # room 0 needs no buffer


def test_the_ledger_handles_use_the_same_stream():
    """RaftAudit.report / RaftWal.poll over fakes: the handle's prefix names
    the entry point, WAL returns (records, info) and keeps its status."""
    fa, fw = FakeEntry(3, abi.AUDIT_EVENT_DTYPE), FakeEntry(2, abi.WAL_RECORD_DTYPE, rc=abi.RAFT_EWINDOW)
    lib = types.SimpleNamespace(raft_last_error=lambda: b"boom", raft_audit_report=fa, raft_audit_report_dev=fa,
                                raft_wal_poll=fw)
    a, w = object.__new__(eng.RaftAudit), object.__new__(eng.RaftWal)
    for h in (a, w):
        h._lib, h._h, h.R, h.G = lib, None, 3, 8
    info, ev = a.report(g0=4)
    assert info == dict(delivered=3, pending=0, flagged=0) and ev["group"].tolist() == [4, 5, 6]
    assert [c[1] for c in fa.calls] == [0, 3]
    with pytest.raises(ValueError, match="16-byte"):
        a.report_dev(0x1008, 2)
    with pytest.raises(ValueError, match="report: max_events"):
        a.report(max_events=True)
    rec, info = w.poll(replica=1)
    assert len(rec) == 2 and info["status"] == abi.RAFT_EWINDOW and info["pending"] == 0
    assert w.peek()["pending"] == 2 and fw.calls[-1] == (None, 0)
    with pytest.raises(ValueError, match="replica"):
        w.poll(replica=3)


def test_the_integer_checker_is_strict_and_names_the_method():
    for bad in (True, 1.0, "1", None, np.bool_(True)):
        with pytest.raises(ValueError, match="m: x must be an integer"):
            eng._int("m", "x", bad)
    assert eng._int("m", "x", np.int32(4)) == 4 and type(eng._int("m", "x", np.int32(4))) is int
    assert eng._int("m", "x", None, allow_none=True) is None
    with pytest.raises(ValueError, match=r"m: x must be None or an integer in 0\.\.3, not 4"):
        eng._int("m", "x", 4, 0, 3, allow_none=True)
    with pytest.raises(ValueError, match="m: x must be an integer >= 1, not 0"):
        eng._int("m", "x", 0, 1)
