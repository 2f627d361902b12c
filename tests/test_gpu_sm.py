"""The replicated state machine on the GPU (marker `gpu`): raft_engine_sm_*
against the plain-Python model of tests/sm_model.py over the oracle's state and
logs.  Every comparison is exact: heads (applied, lost, hash), registers, info."""
import ctypes as C
import importlib

import numpy as np
import pytest

import sm_model as M
from helpers import STRESS_MIX, abi, blank_groups, set_fld
from test_gpu_apply import crafted, same_records

pytestmark = pytest.mark.gpu

eng_mod = importlib.import_module("raft-kotlin_amd.engine")
RaftEngine = eng_mod.RaftEngine
RaftError = eng_mod.RaftError

RING_MIX = dict(log_window=16, cmd_ppm=500_000, drop_ppm=50_000)


def same_machine(e, mach, label="", g0=0, n=None):
    """The device's heads and registers of groups [g0, g0 + n) equal the model's."""
    n = mach.G - g0 if n is None else n
    h, r = e.sm_read(g0, n)
    want = mach.heads(g0, n)
    assert h.dtype == abi.SM_HEAD_DTYPE and r.dtype == np.uint32
    for f in ("applied", "lost", "hash"):
        if not np.array_equal(h[f], want[f]):
            g, q = np.argwhere(h[f] != want[f])[0]
            raise AssertionError(f"{label}: {f} of group {g0 + g} replica {q}: {h[f][g, q]:#x} vs {want[f][g, q]:#x} "
                                 f"({int((h[f] != want[f]).sum())} differ)")
    if not np.array_equal(r, mach.reg[g0:g0 + n]):
        g, q, s = np.argwhere(r != mach.reg[g0:g0 + n])[0]
        raise AssertionError(f"{label}: reg[{s}] of group {g0 + g} replica {q}: {r[g, q, s]:#x} vs "
                             f"{mach.reg[g0 + g, q, s]:#x}")


def test_apply_crafted():
    """The commit > last, commit 0, huge and negative commit clamps, a cursor
    preset through sm_write, two regressed replicas, the replica filter followed
    by the rest, and a second apply that does nothing."""
    R, G, cap, S = 3, 6, 16, 4
    w, t, c = crafted(R, G, cap)
    set_fld(w[1:2], R, 1, "last", 4)                       # commit 6 > lastIndex 4: clamps to 4
    set_fld(w[2:3], R, 0, "commit", 0)                     # nothing committed
    set_fld(w[3:4], R, 2, "commit", 2_000_000_000)         # far beyond the log: clamps to lastIndex
    set_fld(w[4:5], R, 1, "commit", -5)                    # below zero: clamps to 0
    mach = M.Machine(G, R, S)
    mach.applied[0, 1] = 3                                 # preset: applies 3, 4, 5 only, on top of its hash
    mach.hash[0, 1] = 0xFEDCBA9876543210
    mach.reg[0, 1] = (7, 0, 9, 0)
    mach.applied[5, 0] = 6                                 # up to date: nothing
    mach.applied[5, 2] = 7                                 # beyond min(commit, last) = 6: regressed
    mach.applied[4, 1] = 2                                 # hi = 0 < 2: regressed
    with RaftEngine(abi.make_params(R=R, G=G, log_cap=cap)) as e:
        e.write_state(w)
        e.write_log(t, c)
        e.sm_configure(S)
        e.sm_write(mach.heads(), mach.reg)
        same_machine(e, mach, "sm_write")
        # the filter first: replica 1 of groups [1, 5)
        want = M.apply(w, t, c, mach, R, cap, g0=1, n=4, replica=1)
        got = e.sm_apply(1, 4, replica=1)
        assert got == want and got["regressed"] == 1 and got["applied"] == 4 + 6 + 6, (got, want)
        same_machine(e, mach, "replica filter")
        # then everything that is left
        want = M.apply(w, t, c, mach, R, cap)
        got = e.sm_apply()
        assert got == want and got["regressed"] == 2 and got["lost"] == 0 and got["status"] == 0, (got, want)
        same_machine(e, mach, "all")
        h, r = e.sm_read()
        assert h["applied"][0, 1] == 6 and h["applied"][2, 0] == 0 and h["applied"][3, 2] == 8
        assert h["applied"][5, 2] == 7 and h["applied"][4, 1] == 2                 # regressed: unchanged
        assert h["hash"][2, 0] == 0 and not r[2, 0].any()
        assert list(r[0, 0]) == [4, 5, 2, 3]                                       # cmds 0..5 of (0, 0): last writer wins
        assert list(r[0, 1]) == [7, 13, 14, 15]                                    # cmds 13, 14, 15 over the preset
        got = e.sm_apply()
        assert got == dict(applied=0, lost=0, regressed=2, status=0)
        same_machine(e, mach, "second apply")
        assert np.array_equal(e.read_state(), w) and not e.applied().any()         # the drain's cursor is its own


@pytest.mark.parametrize("mode", [0, 1], ids=["reference", "textbook"])
@pytest.mark.parametrize("R", [1, 3, 5, 7, 8])
def test_apply_lockstep(R, mode):
    """Stepped and applied beside the model over the oracle; a drain after every
    second apply shows the two cursors are independent."""
    tb = dict(mode=1, ae_max_entries=4) if mode else {}
    kw = dict(R=R, G=203, seed=11, log_cap=300, **tb, **STRESS_MIX)
    S = 8
    points, (st, t, c, digest), final = M.oracle_run(400, 7, S, drain_every=2, **kw)
    host = M.Machine(203, R, S)
    total = 0
    with RaftEngine(abi.make_params(**kw)) as e:
        e.sm_configure(S)
        for k, (winfo, wheads, wregs, d) in enumerate(points):
            e.step(7, counters=False)
            info = e.sm_apply()
            assert info == winfo, f"R{R} mode{mode} apply {k}: {info} vs {winfo}"
            h, r = e.sm_read()
            assert np.array_equal(h, wheads) and np.array_equal(r, wregs), f"R{R} mode{mode} apply {k}"
            total += info["applied"]
            if d is not None:                              # the drain still sees every entry since ITS cursor
                rec, dinfo = e.drain_committed()
                same_records(rec, d[0], f"R{R} mode{mode} drain {k}")
                assert dinfo == d[1]
                for g, q, i, tm, cm in rec.tolist():
                    host.apply_entry(g, q, i, tm, cm)
        assert total > 0
        assert np.array_equal(e.read_state(), st) and e.digest() == digest        # apply reads the canonical state only
        assert all(np.array_equal(a, b) for a, b in zip(e.read_log(), (t, c)))
        if mode:                                           # textbook: the host fold of the drained records is the machine
            rec, _ = e.drain_committed()
            for g, q, i, tm, cm in rec.tolist():
                host.apply_entry(g, q, i, tm, cm)
            h, r = e.sm_read()
            assert np.array_equal(e.applied(), h["applied"])
            assert np.array_equal(host.hash, h["hash"]) and np.array_equal(host.reg, r)
            assert e.sm_check() == 0 and not M.check(final).any()
        else:
            n, flags = e.sm_check(flags=True)
            assert np.array_equal(flags, M.check(final)) and n == int(flags.sum())


SKEW_LENS = (0, 1, 63, 300, 64, 65, 7, 0, 0, 130)


@pytest.mark.parametrize("S", [1, 8, 64])
def test_apply_skew_and_tile_edges(S):
    """State written directly: a run of 300 entries between runs of 0, 1, 63, 64
    and 65 (runs that straddle the 64-entry batches at every offset), a run
    whose commands all hit one slot and runs that cycle through all 64 slots
    exactly once; selections of 63, 64, 65 and 129 replicas."""
    R, G, cap = 3, 129, 512
    w = blank_groups(G, R)
    rng = np.random.default_rng(17)
    t = rng.integers(1, 50, (G, R, cap), dtype=np.int32)
    c = rng.integers(0, 2 ** 32, (G, R, cap), dtype=np.uint32)
    lens = np.array([SKEW_LENS[j % len(SKEW_LENS)] for j in range(G * R)], np.int32).reshape(G, R)
    one = lens == 300
    c[one] = (c[one] & ~np.uint32(63)) | np.uint32(5)                  # every command of the long runs: one slot
    cyc = (lens == 64) | (lens == 65)
    c[cyc] = (c[cyc] & ~np.uint32(63)) | (np.arange(cap, dtype=np.uint32) & np.uint32(63))   # each of 64 slots once
    for r in range(R):
        set_fld(w, R, r, "last", lens[:, r])
        set_fld(w, R, r, "phys", lens[:, r])
        set_fld(w, R, r, "commit", lens[:, r])
    mach = M.Machine(G, R, S)
    with RaftEngine(abi.make_params(R=R, G=G, log_cap=cap)) as e:
        e.write_state(w)
        e.write_log(t, c)
        e.sm_configure(S)
        # 63 replicas; 64, 65 and 65 by the replica filter; 129 replicas (three tiles, the last of one lane)
        for g0, n, q in ((0, 21, -1), (21, 64, 1), (21, 65, 0), (21, 65, 2), (86, 43, -1), (0, G, -1)):
            want = M.apply(w, t, c, mach, R, cap, g0=g0, n=n, replica=q)
            got = e.sm_apply(g0, n, q)
            assert got == want, f"S{S} selection {(g0, n, q)}: {got} vs {want}"
            same_machine(e, mach, f"S{S} selection {(g0, n, q)}")
        assert np.array_equal(mach.applied, lens) and want["applied"] == lens[85, 1] > 0
        assert e.sm_apply() == dict(applied=0, lost=0, regressed=0, status=0)


@pytest.mark.parametrize("every", [5, 100])
@pytest.mark.parametrize("mode", [0, 1], ids=["reference", "textbook"])
def test_apply_ring(mode, every):
    """log_window 16, rows that wrapped many times: applied every 5 steps nothing
    leaves the window unapplied; every 100 the skipped entries are counted per
    replica and in info, RAFT_EWINDOW comes back after everything else was
    applied, the cursor is past the gap and sm_check ignores those replicas."""
    kw = dict(R=5, G=203, seed=11, log_cap=300, mode=mode, **RING_MIX)
    points, (st, _, _, digest), final = M.oracle_run(400, every, 8, **kw)
    with RaftEngine(abi.make_params(**kw)) as e:
        e.sm_configure(8)
        for k, (winfo, wheads, wregs, _) in enumerate(points):
            e.step(every, counters=False)
            info = e.sm_apply()
            assert info == winfo, f"ring mode{mode} every{every} apply {k}: {info} vs {winfo}"
            h, r = e.sm_read()
            assert np.array_equal(h, wheads) and np.array_equal(r, wregs), f"ring mode{mode} every{every} apply {k}"
        lost = sum(p[0]["lost"] for p in points)
        assert (lost > 0) == (every == 100) and sum(p[0]["applied"] for p in points) > 0
        assert any(p[0]["status"] == abi.RAFT_EWINDOW for p in points) == (every == 100)
        assert int(h["lost"].sum()) == lost and st[:, abi.F_INDEX["phys"]].max() > 16   # wrapped
        n, flags = e.sm_check(flags=True)
        assert np.array_equal(flags, M.check(final)) and n == int(flags.sum())
        assert np.array_equal(e.read_state(), st) and e.digest() == digest


def test_apply_in_pieces_equals_once():
    """Textbook mode, flat log: applying after every step and applying once at
    the end give identical machines, and State Machine Safety holds."""
    kw = dict(R=3, G=130, seed=5, log_cap=300, mode=1, ae_max_entries=4, **STRESS_MIX)
    with RaftEngine(abi.make_params(**kw)) as a, RaftEngine(abi.make_params(**kw)) as b:
        a.sm_configure(16)
        b.sm_configure(16)
        pieces = 0
        for _ in range(150):
            a.step(1, counters=False)
            info = a.sm_apply()
            assert info["regressed"] == 0 and info["status"] == 0
            pieces += info["applied"]
        b.step(150, counters=False)
        once = b.sm_apply()
        assert once["applied"] == pieces > 1000 and a.digest() == b.digest()
        (ha, ra), (hb, rb) = a.sm_read(), b.sm_read()
        assert np.array_equal(ha, hb) and np.array_equal(ra, rb)
        assert a.sm_check() == 0 and b.sm_check() == 0


def test_check_crafted():
    """Equal applied and different hashes are flagged, with the flags byte;
    unequal applied is not, and neither is a replica that lost entries."""
    R, G, S = 3, 5, 2
    h = np.zeros((G, R), abi.SM_HEAD_DTYPE)
    h["applied"][:] = 5
    h["hash"][:] = 0x1111222233334444
    h["hash"][1, 2] = 0x1111222233334445                   # group 1: same cursor, another hash (low word)
    h["hash"][2, 0] = 0x9111222233334444                   # group 2: another hash, but another cursor too
    h["applied"][2, 0] = 4
    h["hash"][3, 1] = 7                                    # group 3: another hash on a replica that lost entries
    h["lost"][3, 1] = 1
    h["hash"][4, 0] = 0x0111222233334444                   # group 4: differs in the high word only
    with RaftEngine(abi.make_params(R=R, G=G, log_cap=16)) as e:
        e.sm_configure(S)
        assert e.sm_check() == 0
        e.sm_write(heads=h)
        n, flags = e.sm_check(flags=True)
        assert n == 2 and list(flags) == [0, 1, 0, 0, 1]
        assert e.sm_check(2, 2) == 0 and e.sm_check(1, 1) == 1 and e.sm_check(0, 0) == 0
        n, flags = e.sm_check(3, 2, flags=True)
        assert n == 1 and list(flags) == [0, 1]
        with pytest.raises(RaftError, match="range"):
            e.sm_check(3, 3)


def test_get():
    """Leader-routed and explicit replicas, a group with no leader, two leaders
    (the lowest), an out-of-range group (RAFT_ERANGE, nothing filled), n = 0."""
    R, G, S = 3, 6, 8
    w = blank_groups(G, R)
    set_fld(w[0:1], R, 1, "role", abi.LEADER)
    set_fld(w[1:2], R, 0, "role", abi.LEADER)
    set_fld(w[1:2], R, 2, "role", abi.LEADER)              # two leaders: the lowest index is read
    set_fld(w[3:4], R, 2, "role", abi.LEADER)
    set_fld(w[4:5], R, 0, "role", abi.CANDIDATE)           # groups 2, 4, 5: no leader
    rng = np.random.default_rng(9)
    for r in range(R):
        set_fld(w, R, r, "commit", rng.integers(0, 9, G))
    mach = M.Machine(G, R, S)
    mach.reg[:] = rng.integers(1, 2 ** 32, (G, R, S), dtype=np.uint32)
    mach.applied[:] = rng.integers(0, 9, (G, R))
    lib = abi.load_library()
    with RaftEngine(abi.make_params(R=R, G=G, log_cap=16)) as e:
        e.write_state(w)
        e.sm_configure(S)
        e.sm_write(mach.heads(), mach.reg)
        groups = [g for g in range(G) for _ in range(4)] + [5, 0]
        keys = [int(k) for k in rng.integers(0, 2 ** 32, len(groups))]
        reps = [-1, 0, 1, 2] * G + [-1, -1]
        got = e.sm_get(groups, keys, reps)
        want = M.get(w, mach, R, groups, keys, reps)
        assert got.dtype == abi.SM_VALUE_DTYPE and np.array_equal(got, want), (got, want)
        assert list(got["replica"][::4][:6]) == [1, 0, -1, 2, -1, -1] and not got["value"][8]
        assert np.array_equal(e.sm_get([0, 1, 2], [3, 3, 3]), M.get(w, mach, R, [0, 1, 2], [3, 3, 3], [-1] * 3))
        assert np.array_equal(e.sm_get([0, 1, 2], [3, 11, 3], 2), M.get(w, mach, R, [0, 1, 2], [3, 11, 3], [2] * 3))
        assert len(e.sm_get([], [])) == 0
        for bad in (G, -1, 2 ** 40):
            with pytest.raises(RaftError, match="outside"):
                e.sm_get([0, bad, 1], [1, 2, 3])
        g = np.array([0, G, 1], np.int64)
        q = np.array([0, 0, R], np.int32)
        k = np.zeros(3, np.uint32)
        out = np.full(3 * 16, 0xAB, np.uint8)
        assert lib.raft_engine_sm_get(e._h, g.ctypes.data, q.ctypes.data, k.ctypes.data, out.ctypes.data, 3) \
            == abi.RAFT_ERANGE and (out == 0xAB).all()
        g[1] = 2                                           # groups fine, replica R is not
        assert lib.raft_engine_sm_get(e._h, g.ctypes.data, q.ctypes.data, k.ctypes.data, out.ctypes.data, 3) \
            == abi.RAFT_ERANGE and (out == 0xAB).all()
        assert lib.raft_engine_sm_get(e._h, None, None, None, None, 0) == abi.RAFT_OK
        assert lib.raft_engine_sm_get(e._h, g.ctypes.data, None, k.ctypes.data, out.ctypes.data, 3) == abi.RAFT_EINVAL
        assert lib.raft_engine_sm_get(e._h, g.ctypes.data, q.ctypes.data, k.ctypes.data, out.ctypes.data, -1) \
            == abi.RAFT_EINVAL


def test_lifecycle():
    """Every sm_* call before configure is RAFT_EINVAL; device_bytes counts the
    machine and trim_staging keeps it; reset zeroes it; sm_write refuses a bad
    cursor with nothing stored; configure again zeroes or resizes."""
    R, G, cap = 3, 300, 64
    lib = abi.load_library()
    with RaftEngine(abi.make_params(R=R, G=G, seed=4, log_cap=cap, cmd_ppm=1_000_000)) as e:
        idle = e.device_bytes
        info, out = abi.raft_sm_info(), C.c_int64()
        buf = np.zeros(G * R * 16, np.uint8)
        i64, i32, u32 = np.zeros(1, np.int64), np.zeros(1, np.int32), np.zeros(1, np.uint32)
        calls = [lambda: lib.raft_engine_sm_apply(e._h, 0, G, -1, C.byref(info)),
                 lambda: lib.raft_engine_sm_read(e._h, 0, G, buf.ctypes.data, None),
                 lambda: lib.raft_engine_sm_write(e._h, 0, G, buf.ctypes.data, None),
                 lambda: lib.raft_engine_sm_get(e._h, i64.ctypes.data, i32.ctypes.data, u32.ctypes.data,
                                                buf.ctypes.data, 1),
                 lambda: lib.raft_engine_sm_check(e._h, 0, G, None, C.byref(out))]
        for call in calls:
            assert call() == abi.RAFT_EINVAL and b"not configured" in lib.raft_last_error()
        for wrapped in (e.sm_apply, e.sm_read, e.sm_check, lambda: e.sm_get([0], [1])):
            with pytest.raises(RaftError, match="not configured"):
                wrapped()
        for bad in (3, 128, -2):
            assert lib.raft_engine_sm_configure(e._h, bad) == abi.RAFT_EINVAL
        assert e.device_bytes == idle
        e.sm_configure(8)
        with_sm = e.device_bytes
        assert with_sm >= idle + G * R * (16 + 8 * 4)
        assert all(call() == abi.RAFT_OK for call in calls)
        e.step(60, counters=False)
        first = e.sm_apply()
        assert first["applied"] > 0 and not e.applied().any()
        e.sm_check()
        e.sm_get([0, 1], [2, 3])
        assert e.device_bytes > with_sm                    # the check's and the read's staging
        e.trim_staging()
        assert e.device_bytes == with_sm                   # the machine is not staging
        h, r = e.sm_read()
        assert int(h["applied"].sum()) == first["applied"] and r.any() and h["hash"].any()
        # a bad cursor: refused, nothing stored (not even the good heads before it)
        for field, v in (("applied", cap + 1), ("applied", -1), ("lost", -1)):
            bad = np.zeros((G, R), abi.SM_HEAD_DTYPE)
            bad[field][G - 1, R - 1] = v
            assert lib.raft_engine_sm_write(e._h, 0, G, bad.ctypes.data, None) == abi.RAFT_EINVAL
        h2, r2 = e.sm_read()
        assert np.array_equal(h, h2) and np.array_equal(r, r2)
        with pytest.raises(RaftError, match="range"):
            e.sm_read(1, G)
        with pytest.raises(RaftError, match="range"):
            e.sm_apply(G, 1)
        assert lib.raft_engine_sm_apply(e._h, 0, G, R, C.byref(info)) == abi.RAFT_EINVAL
        assert lib.raft_engine_sm_apply(e._h, 0, G, -1, None) == abi.RAFT_EINVAL
        e.reset()
        h, r = e.sm_read()
        assert not h["applied"].any() and not h["hash"].any() and not r.any() and e.device_bytes == with_sm
        e.step(60, counters=False)
        assert e.sm_apply() == first                       # the same run from the same start
        e.sm_configure(8)                                  # again: zeroed
        assert not e.sm_read()[0]["applied"].any() and e.device_bytes == with_sm
        e.sm_configure(64)                                 # another size: reallocated
        assert e.sm_read()[1].shape == (G, R, 64) and e.device_bytes > with_sm
        assert e.sm_apply()["applied"] == first["applied"]
        e.sm_configure(0)
        assert e.device_bytes == idle and e.sm_slots == 0
        assert calls[0]() == abi.RAFT_EINVAL and b"not configured" in lib.raft_last_error()
        e.reset()                                          # reset without a machine: as before


def test_resume_equals_the_uninterrupted_run():
    """sm_read -> a new engine -> write_state / write_log / sm_write -> continue."""
    kw = dict(R=5, G=100, seed=8, log_cap=300, **STRESS_MIX)
    with RaftEngine(abi.make_params(**kw)) as a, RaftEngine(abi.make_params(**kw)) as b:
        a.sm_configure(8)
        for _ in range(5):
            a.step(20, counters=False)
            a.sm_apply()
        heads, regs = a.sm_read()
        assert heads["applied"].any()
        b.write_state(a.read_state())
        b.write_log(*a.read_log())
        b.step_index = a.step_index
        b.sm_configure(8)
        b.sm_write(heads[:40], regs[:40])                  # in two slices of groups
        b.sm_write(heads[40:], regs[40:], g0=40)
        for _ in range(5):
            a.step(20, counters=False)
            b.step(20, counters=False)
            assert a.sm_apply() == b.sm_apply()
        (ha, ra), (hb, rb) = a.sm_read(), b.sm_read()
        assert np.array_equal(ha, hb) and np.array_equal(ra, rb) and a.digest() == b.digest()
        assert (ha["applied"] > heads["applied"]).any()


def test_service_apply_and_read():
    """apply_committed, read (routed to the leader, named by the command table)
    and RaftNode.machine: string commands land in the slot their interned id's
    low bits name."""
    svc_mod = importlib.import_module("raft-kotlin_amd.service")
    R = 3
    w = blank_groups(2, R)
    for r in range(R):
        set_fld(w, R, r, "term", 1)
    set_fld(w, R, 0, "role", abi.LEADER)
    with RaftEngine(abi.make_params(R=R, G=2, log_cap=16)) as e:
        e.write_state(w)
        e.sm_configure(4)
        svc = svc_mod.RaftService(e)
        leader = svc.node(1, 0)
        for s in ("set x 1", "set y 2", "del x"):          # ids BASE + 0, 1, 2: slots 0, 1, 2
            leader.appendCommand(s)
        assert svc.apply_committed() == dict(applied=0, lost=0, regressed=0, status=0)     # appended, not committed
        s = e.read_state()
        set_fld(s[1:2], R, 0, "commit", 2)
        e.write_state(s)
        assert svc.apply_committed()["applied"] == 2
        assert svc.read([1, 1, 1], ["set x 1", "set y 2", "del x"]) == [
            ("set x 1", 0, 2, 2), ("set y 2", 0, 2, 2), ("cmd#00000000", 0, 2, 2)]
        assert svc.read([1], ["set x 1"], replica=1) == [("cmd#00000000", 1, 0, 0)]
        with pytest.raises(KeyError):                      # never submitted: no id, no register, nothing interned
            svc.read([1], ["get z"])
        assert svc.commands.lookup("get z") is None
        head, regs = leader.machine()
        base = svc_mod.CommandTable.BASE
        assert head["applied"] == 2 and head["lost"] == 0 and list(regs) == [base, base + 1, 0, 0]
        assert int(head["hash"]) == M.fold([M.x_of(0, 1, base), M.x_of(1, 1, base + 1)])
        assert svc.node(1, 1).machine()[0]["applied"] == 0 and leader.lastApplied == 0
