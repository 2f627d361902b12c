"""The leader watch on the CPU: the model (watch_model.py) on crafted states and
over the oracle -- what test_gpu_watch.py holds the engine's kernels to -- the
coverage of the parity scenario, and the argument checks of abi.py and the
wrappers.  No device is touched."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

import watch_model as WM
from helpers import abi, fld

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIVES = [c for c in WM.PARITY_CASES if (c[0], c[1]) == (5, 203)]


def test_crafted_groups_give_the_records_written_out_by_hand():
    """No leader, one leader, two LEADERs of different terms with the older at
    the lower index, two of equal terms, the same replica re-elected, a leader
    lost, an unchanged group: events, info and `seen` afterwards."""
    w, seen = WM.crafted()
    assert WM.current(w, WM.CR).tolist() == [[-1, 0], [1, 3], [2, 3], [1, 3], [1, 5], [-1, 0], [0, 3]]
    info, ev, rc = WM.poll(w, seen, WM.CR)
    assert rc == abi.RAFT_OK and info == WM.CRAFTED_INFO
    for name, a, b in zip([WM.CRAFTED_NAMES[g] for g in WM.CRAFTED_EVENTS["group"]], ev.tolist(),
                          WM.CRAFTED_EVENTS.tolist()):
        assert a == b, (name, a, b)
    assert len(ev) == len(WM.CRAFTED_EVENTS) and np.array_equal(seen, WM.CRAFTED_SEEN_AFTER)
    # polled again at once: nothing changed, the leaderless groups are still counted
    info, ev, _ = WM.poll(w, seen, WM.CR)
    assert len(ev) == 0 and info == dict(dict.fromkeys(abi.WATCH_INFO_FIELDS, 0), leaderless=2)
    # a part of the range: groups [2, 5) alone, engine-local group ids
    w, seen = WM.crafted()
    info, ev, _ = WM.poll(w, seen, WM.CR, 2, 3)
    assert ev.tolist() == WM.CRAFTED_EVENTS[1:4].tolist()
    assert info == dict(delivered=3, pending=0, gained=1, lost=0, moved=1, reterm=1, leaderless=0)
    assert np.array_equal(seen[[0, 1, 5, 6]], WM.crafted()[1][[0, 1, 5, 6]])


def test_a_single_replica_group():
    w, seen = WM.crafted_single()
    info, ev, rc = WM.poll(w, seen, 1)
    assert rc == abi.RAFT_OK and info == WM.CRAFTED_SINGLE_INFO and ev.tolist() == WM.CRAFTED_SINGLE_EVENTS.tolist()


def test_the_kinds_partition_the_changed_groups():
    for prev in range(-1, 3):
        for cur in range(-1, 3):
            kinds = [k for k in WM.KINDS if WM.kind_of(cur, prev) == k]
            assert len(kinds) == 1
    assert [WM.kind_of(1, -1), WM.kind_of(-1, 1), WM.kind_of(2, 1), WM.kind_of(1, 1)] == list(WM.KINDS)


@pytest.mark.parametrize("R,G,variant", FIVES, ids=[c[2] for c in FIVES])
def test_the_parity_scenario_covers_the_kinds(R, G, variant):
    """The coverage condition of the run test_gpu_watch.py repeats on the GPU, on
    the oracle, for the (5, 203) shapes.  Every poll point leaves at least one
    group unchanged; the first finds at least 66 changed groups, so that a cut
    can fall in a later wave.  Which kinds a poll point can show follows from
    the watch: before the first report every pair is (-1, 0), so the first poll
    can only gain; lost, moved and gained all occur within the 3 steps to the
    second; a reterm needs the same replica to lose an election round and win a
    later one, which takes more than one election timeout (10 heartbeats) and
    so shows only at the third poll, 20 steps and a restart later, where all
    four kinds occur."""
    points = WM.host_parity_run(R, G, variant)
    infos = [p["info"] for p in points]
    ranges = [G - 5, G - 5, G]
    for info, n, p in zip(infos, ranges, points):
        changed = sum(info[k] for k in WM.KINDS)
        assert info["delivered"] == changed == len(p["events"]) and info["pending"] == 0
        assert changed < n, (p["what"], "no unchanged group")
        assert 0 < info["leaderless"] < n
    assert infos[0]["gained"] >= 66 and all(infos[0][k] == 0 for k in ("lost", "moved", "reterm"))
    assert all(infos[1][k] > 0 for k in ("gained", "lost", "moved")), infos[1]
    assert all(infos[2][k] > 0 for k in WM.KINDS), infos[2]
    # the third poll covers groups the first two never reported (0..2 and the last two)
    edge = np.isin(points[2]["events"]["group"], [0, 1, 2, G - 2, G - 1])
    assert edge.any() and (points[2]["events"]["prev_leader"][edge] == -1).all()
    # a deposed leader at a lower index than its successor: the case raft_leader_info.leader gets wrong
    st = points[2]["state"]
    cur = WM.current(st, R)
    lowest = np.array([min([r for r in range(R) if fld(st, R, r, "role")[g] == abi.LEADER], default=-1)
                       for g in range(G)])
    assert (lowest != cur[:, 0]).any()
    # the watch ends at the directory of the state
    assert np.array_equal(points[2]["watch"], cur)


@pytest.mark.parametrize("R,G,variant", [(5, 203, "flat"), (1, 70, "flat")])
def test_successive_polls_concatenate_for_every_cut(R, G, variant):
    """With no step in between, polls of max_events each concatenated equal one
    poll with enough room, for every max_events from 1 to the total; the kind
    counts describe the whole range at each call; `seen` advances only for the
    groups that were written."""
    h = WM.Host(**WM.parity_kw(R, G, variant))
    h.step(WM.WARM_STEPS)
    st = h.read_state()
    h.close()
    g0, n = 3, G - 5
    cur = WM.current(st, R)
    whole_seen = WM.fresh(G)
    whole_info, whole, _ = WM.poll(st, whole_seen, R, g0, n)
    total = len(whole)
    assert total >= (66 if R == 5 else 2)
    for m in range(1, total + 1):
        seen = WM.fresh(G)
        got, at = [], 0
        while True:
            info, ev, rc = WM.poll(st, seen, R, g0, n, m, cur=cur)
            assert rc == abi.RAFT_OK and info["delivered"] == len(ev) == min(m, total - at)
            at += len(ev)
            assert info["pending"] == total - at
            assert sum(info[k] for k in WM.KINDS) == info["delivered"] + info["pending"]
            assert info["leaderless"] == whole_info["leaderless"]
            got.append(ev)
            # reported so far: exactly the groups of the events so far
            want_seen = WM.fresh(G)
            done = whole[:at]
            want_seen[done["group"], 0], want_seen[done["group"], 1] = done["leader"], done["term"]
            assert np.array_equal(seen, want_seen)
            if info["pending"] == 0:
                break
        assert np.array_equal(np.concatenate(got), whole), m
        assert np.array_equal(seen, whole_seen)
    # max_events 0 with a buffer delivers nothing and stores nothing
    seen = WM.fresh(G)
    info, ev, _ = WM.poll(st, seen, R, g0, n, 0)
    assert len(ev) == 0 and info["pending"] == total and np.array_equal(seen, WM.fresh(G))


def test_a_peek_stores_nothing():
    w, seen = WM.crafted()
    before = seen.copy()
    info, ev, rc = WM.poll(w, seen, WM.CR, peek=True)
    assert rc == abi.RAFT_OK and len(ev) == 0 and np.array_equal(seen, before)
    assert info == dict(WM.CRAFTED_INFO, delivered=0, pending=5)
    h = WM.Host(**WM.parity_kw(3, 23, "flat"))
    h.step(WM.WARM_STEPS)
    peek, _ = h.poll_leaders(peek=True)
    assert np.array_equal(h.read_watch(), WM.fresh(23))
    info, ev = h.poll_leaders()
    assert peek["pending"] == info["delivered"] == len(ev) > 0
    assert {k: peek[k] for k in WM.KINDS + ("leaderless",)} == {k: info[k] for k in WM.KINDS + ("leaderless",)}
    h.close()


def test_model_return_codes():
    w, seen = WM.crafted()
    G = len(w)
    for g0, n in ((G, 1), (-1, 2), (G - 1, 2), (0, -1)):
        assert WM.poll(w, seen, WM.CR, g0, n)[2] == abi.RAFT_ERANGE
    assert WM.poll(w, seen, WM.CR, 0, G, -1)[2] == abi.RAFT_EINVAL
    info, ev, rc = WM.poll(w, seen, WM.CR, G, 0)
    assert rc == abi.RAFT_OK and len(ev) == 0 and info == dict.fromkeys(abi.WATCH_INFO_FIELDS, 0)
    assert np.array_equal(seen, WM.crafted()[1])


def test_write_watch_validation():
    """Every leader in -1..R-1, every term >= 0, a leader of -1 with term 0
    only: the model's rule and the wrapper's, before any library call."""
    good = [[(-1, 0)], [(0, 0)], [(2, 7)], [(0, 2 ** 31 - 1)], [(-1, 0), (1, 1)]]
    bad = [[(-2, 0)], [(3, 1)], [(1, -1)], [(-1, 1)], [(0, 1), (-1, 5)]]
    for pairs in good:
        assert WM.valid_watch(pairs, 3), pairs
    for pairs in bad:
        assert not WM.valid_watch(pairs, 3), pairs
    h = WM.Host(**WM.parity_kw(3, 23, "flat"))
    h.write_watch(np.array([(2, 7), (-1, 0)], np.int32), g0=4)
    assert h.read_watch(4, 2).tolist() == [[2, 7], [-1, 0]] and h.read_watch(3, 1).tolist() == [[-1, 0]]
    with pytest.raises(ValueError):
        h.write_watch(np.array([(3, 1)], np.int32))
    h.close()
    e = object.__new__(importlib.import_module("raft-kotlin_amd.engine").RaftEngine)
    e.R, e.G, e._h = 3, 8, None
    for pairs in bad:
        with pytest.raises(ValueError, match="write_watch"):
            e.write_watch(np.array(pairs, np.int64))
    for shape in (np.zeros((2, 3), np.int32), np.zeros(4, np.int32), np.zeros((2, 2), np.float32)):
        with pytest.raises(ValueError, match="write_watch"):
            e.write_watch(shape)


def test_wrapper_argument_checks():
    """poll_leaders / poll_leaders_dev refuse what is not an integer, a negative
    max_events and a misaligned device buffer before any library call."""
    e = object.__new__(importlib.import_module("raft-kotlin_amd.engine").RaftEngine)
    e.R, e.G, e._h = 3, 8, None
    for bad in (dict(g0=1.5), dict(n=True), dict(max_events=-1), dict(max_events=2.0), dict(max_events=True)):
        with pytest.raises(ValueError, match="poll_leaders"):
            e.poll_leaders(**bad)
    with pytest.raises(ValueError, match="8-byte"):
        e.poll_leaders_dev(0x1004, 4)
    with pytest.raises(ValueError, match="required"):
        e.poll_leaders_dev(0, 4)
    with pytest.raises(ValueError, match="max_events"):
        e.poll_leaders_dev(0x1000, -1)


def test_abi_symbols_and_record_sizes():
    lib = abi.load_library()
    assert C.sizeof(abi.raft_leader_event) == 24 == abi.EVENT_DTYPE.itemsize
    assert C.sizeof(abi.raft_watch_info) == 64 == abi.WATCH_INFO_DTYPE.itemsize
    hdr = open(os.path.join(ROOT, "include", "raft_engine.h")).read()
    for struct, dtype in ((abi.raft_leader_event, abi.EVENT_DTYPE), (abi.raft_watch_info, abi.WATCH_INFO_DTYPE)):
        m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct.__name__, struct.__name__), hdr, re.S)
        names = re.findall(r"int(?:32|64)_t\s+(\w+);", m.group(1))
        assert names == [n for n, _ in struct._fields_] == list(dtype.names)
        assert [dtype.fields[n][1] for n in names] == [getattr(struct, n).offset for n in names]
    assert list(abi.WATCH_INFO_FIELDS) == list(abi.WATCH_INFO_DTYPE.names[:-1])
    for name in ("raft_engine_poll_leaders", "raft_engine_poll_leaders_dev", "raft_engine_read_watch",
                 "raft_engine_write_watch"):
        assert name in abi.EXPORTED_SYMBOLS and getattr(lib, name).restype is C.c_int
    assert lib.raft_abi_version() == 2
    B = importlib.import_module("raft-kotlin_amd.build")
    assert any(os.path.basename(s) == "raft_watch.hip" for s in B.SRCS)          # raft_build_source_id covers it


def test_einval_without_a_device():
    """A null engine is refused by every entry point before anything else."""
    lib = abi.load_library()
    info = abi.raft_watch_info()
    buf = np.zeros(64, np.int32)
    p = C.c_void_p(buf.ctypes.data)
    for fn in (lib.raft_engine_poll_leaders, lib.raft_engine_poll_leaders_dev):
        assert fn(None, 0, 2, p, 2, C.byref(info)) == abi.RAFT_EINVAL and b"null engine" in lib.raft_last_error()
    for fn in (lib.raft_engine_read_watch, lib.raft_engine_write_watch):
        assert fn(None, 0, 2, abi.ptr(buf, C.c_int32)) == abi.RAFT_EINVAL and b"null engine" in lib.raft_last_error()


def test_a_library_without_the_symbols_gets_stubs(monkeypatch):
    """An experimental library (RAFT_ENGINE_LIB) built before the watch binds a
    stub for each of its entry points that says so when called (here: the
    oracle's library, which exports none of them)."""
    other = os.path.join(ROOT, "oracle", "lib", "liboracle.so")
    assert os.path.exists(other), "the oracle library is built with the package"
    monkeypatch.setenv("RAFT_ENGINE_LIB", other)
    with pytest.warns(UserWarning) as rec:
        lib = abi.load_library(other)
    assert any("no raft_engine_poll_leaders;" in str(w.message) for w in rec)
    for name in ("raft_engine_poll_leaders", "raft_engine_poll_leaders_dev", "raft_engine_read_watch",
                 "raft_engine_write_watch"):
        with pytest.raises(RuntimeError, match=f"{name} is not in this engine build"):
            getattr(lib, name)(None)
