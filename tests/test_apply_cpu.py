"""Committed-entry delivery (lastApplied, raft_engine_drain_committed) without a
GPU: the new entry points' argument checks, the record layouts, the wrappers'
checks on an unbound engine, and the plain-Python model (tests/apply_model.py)
over the oracle on the inputs the GPU tests compare the kernels against."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import apply_model as M
from helpers import STRESS_MIX, abi

ENTRY_POINTS = ["raft_engine_drain_committed", "raft_engine_drain_committed_dev", "raft_engine_read_applied",
                "raft_engine_write_applied"]

# the inputs of the model runs: (steps, drained every, raft_params)
FLAT_REF = (400, 7, dict(R=5, G=200, seed=11, log_cap=300, **STRESS_MIX))
FLAT_TB = (400, 7, dict(R=5, G=200, seed=11, log_cap=300, mode=1, ae_max_entries=4, **STRESS_MIX))
FLAT_TB3 = (400, 50, dict(R=3, G=200, seed=12, log_cap=300, mode=1, **STRESS_MIX))
RING = dict(R=5, G=200, seed=11, log_cap=300, log_window=16, cmd_ppm=500_000, drop_ppm=50_000)
RING_OFTEN, RING_RARELY = (400, 5, RING), (400, 100, RING)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(abi.LIB_PATH):
        importlib.import_module("raft-kotlin_amd.build").build()
    return abi.load_library()


def test_record_layouts():
    assert C.sizeof(abi.raft_applied_entry) == 24 and C.sizeof(abi.raft_drain_info) == 32
    assert abi.APPLIED_DTYPE.itemsize == 24
    assert [abi.APPLIED_DTYPE.fields[f][1] for f in ("group", "replica", "index", "term", "cmd")] == [0, 8, 12, 16, 20]
    assert set(ENTRY_POINTS) <= set(abi.EXPORTED_SYMBOLS)


def test_entry_points_check_arguments_before_any_device_call(lib):
    info = abi.raft_drain_info()
    buf = np.zeros(4, abi.APPLIED_DTYPE)
    for fn in (lib.raft_engine_drain_committed, lib.raft_engine_drain_committed_dev):
        assert fn(None, 0, 1, -1, buf.ctypes.data, 4, C.byref(info)) == abi.RAFT_EINVAL
        assert b"null engine" in lib.raft_last_error()
        assert fn(None, 0, 1, 9, None, 0, None) == abi.RAFT_EINVAL
    a = np.zeros((1, 5), np.int32)
    assert lib.raft_engine_read_applied(None, 0, 1, abi.ptr(a, C.c_int32)) == abi.RAFT_EINVAL
    assert lib.raft_engine_write_applied(None, 0, 1, abi.ptr(a, C.c_int32)) == abi.RAFT_EINVAL


def _unbound_engine(R=5, cap=8):
    """A RaftEngine shell without a device handle or library (as test_abi.py's):
    a wrapper that gets past its own checks fails on the missing library."""
    eng = importlib.import_module("raft-kotlin_amd.engine")
    e = object.__new__(eng.RaftEngine)
    e.R, e.cap, e.G, e._h = R, cap, 4, None
    return e


def test_wrappers_reject_bad_arguments_before_any_library_call():
    e = _unbound_engine(R=3, cap=8)
    for bad in (dict(replica=3), dict(replica=-2), dict(max_entries=-1), dict(max_entries=2.5), dict(g0=0.5)):
        with pytest.raises(ValueError):
            e.drain_committed(**bad)
    with pytest.raises(ValueError):
        e.peek_committed(replica=3)
    with pytest.raises(ValueError):
        e.drain_committed_dev(0, 8)                       # room without a buffer
    with pytest.raises(ValueError):
        e.drain_committed_dev(1028, 8)                    # records hold an int64: 8-byte aligned
    with pytest.raises(ValueError):
        e.drain_committed_dev(1024, 8, replica=3)
    for bad in (np.zeros((4, 2), np.int32), np.zeros(12, np.int32), np.zeros((4, 3), np.float32),
                np.full((4, 3), 9, np.int32), np.full((4, 3), -1, np.int32)):
        with pytest.raises(ValueError):
            e.set_applied(bad)
    with pytest.raises(AttributeError):                   # a good call reaches the (absent) library
        e.set_applied(np.full((4, 3), 8, np.int32))


def _run(case):
    steps, every, kw = case
    return M.oracle_run(steps, every, **kw)[0], kw


def test_model_flat_log_reference_mode():
    """Nothing is ever lost on a flat log; the reference's quirks do lower
    min(commitIndex, lastIndex) below lastApplied (regressions are observed)."""
    d, kw = _run(FLAT_REF)
    t = M.totals(d)
    assert t["delivered"] > 0 and t["lost"] == 0 and t["regressed"] > 0, t
    assert all(info["status"] == abi.RAFT_OK for _, info, _ in d)


@pytest.mark.parametrize("case", [FLAT_TB, FLAT_TB3], ids=["R5-E4-every7", "R3-every50"])
def test_model_textbook_streams_are_prefixes(case):
    d, kw = _run(case)
    t = M.totals(d)
    assert t["delivered"] > 0 and t["lost"] == 0 and t["regressed"] == 0, t
    assert M.prefix_violations(d, kw["G"], kw["R"]) == 0


def test_model_ring_loses_entries_only_when_rarely_drained():
    often, _ = _run(RING_OFTEN)
    rarely, _ = _run(RING_RARELY)
    to, tr = M.totals(often), M.totals(rarely)
    assert to["delivered"] > 0 and to["lost"] == 0, to
    assert tr["delivered"] > 0 and tr["lost"] > 0, tr
    assert any(info["status"] == abi.RAFT_EWINDOW for _, info, _ in rarely)


def test_model_room_and_peek():
    """Drains with little room concatenate to one drain; a peek stores nothing."""
    steps, every, kw = FLAT_REF
    _, (st, t, c, _) = M.oracle_run(steps, every, **kw)
    R, G, cap = kw["R"], kw["G"], kw["log_cap"]
    a0 = np.zeros((G, R), np.int64)
    whole, info = M.drain(st, t, c, a0, R, cap)
    a1 = np.zeros((G, R), np.int64)
    _, pk = M.drain(st, t, c, a1, R, cap, peek=True)
    assert pk["pending"] == len(whole) and pk["delivered"] == 0 and not a1.any()
    parts = []
    while True:
        rec, inf = M.drain(st, t, c, a1, R, cap, room=997)
        parts.append(rec)
        assert inf["pending"] == len(whole) - sum(len(p) for p in parts)
        if not inf["pending"]:
            break
    assert np.array_equal(np.concatenate(parts), whole) and np.array_equal(a0, a1)
