"""The leader watch on the GPU (marker `gpu`): raft_engine_poll_leaders* and
raft_engine_read_watch / write_watch against tests/watch_model.py, over the
oracle's state where the oracle run is valid and over the engine's own exported
state everywhere.  Every comparison is exact."""
import ctypes as C
import importlib

import numpy as np
import pytest

import restart_model as RM
import watch_model as WM
from helpers import abi, assert_same_state, blank_groups, high_g0, set_fld

pytestmark = pytest.mark.gpu

eng_mod = importlib.import_module("raft-kotlin_amd.engine")
service = importlib.import_module("raft-kotlin_amd.service")
RaftEngine = eng_mod.RaftEngine
RaftError = eng_mod.RaftError


def same(got, want, label=""):
    assert got.dtype == want.dtype and len(got) == len(want), (label, got.dtype, len(got), len(want))
    if not np.array_equal(got, want):
        at = int(np.nonzero(got != want)[0][0])
        raise AssertionError(f"{label}: {int((got != want).sum())} records differ; first at {at}: {got[at]} vs {want[at]}")


class Shadow:
    """A RaftEngine whose every poll is checked, as it happens, against the
    model over the engine's own exported state and a `seen` array carried
    here: events, info and read_watch."""

    def __init__(self, e):
        self.e, self.seen = e, WM.fresh(e.G)

    def __getattr__(self, name):
        return getattr(self.e, name)

    def poll_leaders(self, g0=0, n=None, max_events=None, peek=False):
        want_info, want_ev, rc = WM.poll(self.e.read_state(), self.seen, self.e.R, g0, n, max_events, peek)
        assert rc == abi.RAFT_OK
        info, ev = self.e.poll_leaders(g0, n, max_events, peek)
        assert info == want_info, (info, want_info)
        same(ev, want_ev, f"events of [{g0}, +{n}) max {max_events}")
        assert np.array_equal(self.e.read_watch(), self.seen), "seen differs from the model's"
        return info, ev


def assert_same_points(got, want, quiet, R):
    """Every checkpoint of the engine's parity_run equals the model's over the
    oracle, bit for bit, as long as the oracle run is valid (on a ring, up to its
    first window miss: restart_model.assert_same_rows); and the steps in
    between left what they leave on an engine that never polled."""
    assert len(got) == len(want) == len(quiet)
    for a, q in zip(got, quiet):
        assert np.array_equal(a["counters"], q["counters"]), f"{a['what']}: counter rows differ from the unpolled engine's"
        assert a["digest"] == q["digest"], f"{a['what']}: digest differs from the unpolled engine's"
    for a, b in zip(got, want):
        label = b["what"]
        if not RM.assert_same_rows(a["counters"], b["counters"], label):
            return
        assert_same_state(a["state"], b["state"], R, label)
        assert a["info"] == b["info"], f"{label}: info {a['info']} vs {b['info']}"
        same(a["events"], b["events"], f"{label}: events")
        assert np.array_equal(a["watch"], b["watch"]), f"{label}: read_watch differs"
        assert a["digest"] == b["digest"], label


@pytest.mark.parametrize("R,G,variant", WM.PARITY_CASES, ids=[f"R{c[0]}-G{c[1]}-{c[2]}" for c in WM.PARITY_CASES])
def test_parity_with_the_model(R, G, variant):
    """40 steps, a poll over [3, G - 2), 3 steps, a poll, a restart with
    down_steps, 20 steps, a poll over everything: events, info and read_watch
    equal the model's, and the digest and the counter rows of the steps in
    between equal those of an engine that never polled."""
    want = WM.host_parity_run(R, G, variant)
    kw = WM.parity_kw(R, G, variant)
    with RaftEngine(abi.make_params(**kw)) as e, RaftEngine(abi.make_params(**kw)) as q:
        got = WM.parity_run(Shadow(e), f"R{R} G{G} {variant}")
        quiet = WM.parity_run(q, "unpolled", poll=False)
        assert q.device_bytes < e.device_bytes                  # `seen` counts, and only once it is in use
    assert_same_points(got, want, quiet, R)


@pytest.mark.parametrize("where,variant", [("bit31", "ring"), ("top", "flat")])
def test_parity_at_the_top_of_the_global_ids(where, variant):
    """A shard that straddles global id 2^31, and one whose last group is
    2^32 - 1: events name engine-local groups."""
    g0 = high_g0(203)[where]
    want = WM.host_parity_run(5, 203, variant, g0)
    kw = dict(WM.parity_kw(5, 203, variant), g0=g0)
    with RaftEngine(abi.make_params(**kw)) as e, RaftEngine(abi.make_params(**kw)) as q:
        got = WM.parity_run(Shadow(e), f"R5 G203 {variant} {where}")
        quiet = WM.parity_run(q, "unpolled", poll=False)
    assert_same_points(got, want, quiet, 5)
    ev = got[2]["events"]
    assert len(ev) > 0 and ev["group"].min() >= 0 and ev["group"].max() < 203


@pytest.mark.parametrize("R,G", [(5, 203), (1, 70)])
def test_the_cut(R, G):
    """max_events in {1, 63, 64, 65, total - 1, total} over [3, G - 2) -- at
    (1, 70) the range crosses a wave boundary with a partial last wave --
    drained to pending == 0: the concatenation equals one poll with enough
    room, and `seen` after each partial poll is the model's."""
    kw = WM.parity_kw(R, G, "flat")
    g0, n = 3, G - 5
    with RaftEngine(abi.make_params(**kw)) as e:
        e.step(WM.WARM_STEPS, counters=False)
        st = e.read_state()
        whole_info, whole, rc = WM.poll(st, WM.fresh(G), R, g0, n)
        total = len(whole)
        assert total > 64 and n > 64                                # a cut can fall on and beyond the wave boundary
        for m in WM.cuts(total):
            e.write_watch(WM.fresh(G))
            # a poll with a buffer and no room delivers nothing and stores nothing
            buf = np.zeros(1, abi.EVENT_DTYPE)
            wi = abi.raft_watch_info()
            assert e._lib.raft_engine_poll_leaders(e._h, g0, n, C.c_void_p(buf.ctypes.data), 0, C.byref(wi)) == abi.RAFT_OK
            assert (wi.delivered, wi.pending) == (0, total) and np.array_equal(e.read_watch(), WM.fresh(G))
            s = Shadow(e)
            infos, events, watches = WM.drain(s, g0, n, m)
            same(np.concatenate(events), whole, f"max_events {m}")
            assert len(infos) == -(-total // m) and [len(x) for x in events[:-1]] == [m] * (len(infos) - 1)
            assert {k: infos[0][k] for k in WM.KINDS} == {k: whole_info[k] for k in WM.KINDS}
            for info in infos:                                      # the counts describe the range at each call
                assert sum(info[k] for k in WM.KINDS) == info["delivered"] + info["pending"]
                assert info["leaderless"] == whole_info["leaderless"]


def test_past_one_workgroup_and_a_partial_last_wave():
    """G = 70,001, R = 3 (the audit's test of this name, for the other user of
    the shared stream kernels): a state built in numpy and loaded with
    write_state, never stepped.  Groups [0, 640) all have a leader (waves of 64
    hits: rank 63), [640, 1280) none (waves with no hit), from 1280 on every
    7th.  [3, G - 2) polled with room for everything, in two parts cut at half,
    and in the _dev form: events, info and read_watch are the model's."""
    import torch
    R, G = 3, 70_001
    g0, n = 3, G - 5
    g = np.arange(G)
    led = (g < 640) | ((g >= 1280) & ((g - 1280) % 7 == 0))
    w = blank_groups(G, R)
    for r in range(R):
        mine = led & (g % R == r)
        rows = w[mine]                                              # (a boolean index copies: stored back below)
        set_fld(rows, R, r, "role", abi.LEADER)
        set_fld(rows, R, r, "term", 1 + g[mine] % 5)
        w[mine] = rows
    # by arithmetic: 637 groups of [3, 640), and 1280 + 7 k < G - 2 for k = 0 .. 9816
    total = 637 + 9817
    assert total == 10_454 == int(led[g0:g0 + n].sum())
    cur = WM.current(w, R)
    want_info, want_ev, rc = WM.poll(w, WM.fresh(G), R, g0, n, cur=cur)
    assert rc == abi.RAFT_OK and len(want_ev) == total
    assert want_info == dict(delivered=total, pending=0, gained=total, lost=0, moved=0, reterm=0, leaderless=n - total)
    with RaftEngine(abi.make_params(R=R, G=G, log_cap=16)) as e:
        e.write_state(w)
        # once, with room for everything
        seen = WM.fresh(G)
        assert WM.poll(w, seen, R, g0, n, cur=cur)[0] == want_info
        info, ev = e.poll_leaders(g0, n)
        assert info == want_info
        same(ev, want_ev, "one poll")
        assert np.array_equal(e.read_watch(), seen)
        # from a fresh seen in two parts
        e.write_watch(WM.fresh(G))
        seen, parts = WM.fresh(G), []
        for room in (total // 2, total):
            m_info, m_ev, _ = WM.poll(w, seen, R, g0, n, room, cur=cur)
            info, ev = e.poll_leaders(g0, n, room)
            assert info == m_info, (room, info, m_info)
            same(ev, m_ev, f"max_events {room}")
            assert np.array_equal(e.read_watch(), seen)
            parts.append(ev)
        assert [len(p) for p in parts] == [total // 2, total - total // 2]
        same(np.concatenate(parts), want_ev, "the two parts")
        # the _dev form
        e.write_watch(WM.fresh(G))
        buf = torch.full(((total + 1) * 6,), -7, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        assert e.poll_leaders_dev(buf.data_ptr(), total, g0, n) == want_info
        raw = buf.cpu().numpy()
        same(raw[:total * 6].view(abi.EVENT_DTYPE), want_ev, "device events")
        assert (raw[total * 6:] == -7).all()
        assert np.array_equal(e.read_watch(), seen)


def test_host_device_and_peek_forms_agree():
    """Three engines in one state: the host form, the _dev form, a peek.  The
    same info and records; the _dev form writes nothing beyond its records, with
    room to spare and at a cut; a misaligned buffer is refused; a peek leaves
    read_watch unchanged."""
    import torch
    R, G = 5, 203
    kw = WM.parity_kw(R, G, "flat")
    g0, n = 3, G - 5
    with RaftEngine(abi.make_params(**kw)) as a, RaftEngine(abi.make_params(**kw)) as d, \
            RaftEngine(abi.make_params(**kw)) as p:
        for e in (a, d, p):
            e.step(WM.WARM_STEPS, counters=False)
        dg = a.digest()
        info, ev = a.poll_leaders(g0, n)
        total = info["delivered"]
        assert total > 70 and info["pending"] == 0
        peek, none = p.poll_leaders(g0, n, peek=True)
        assert peek == dict(info, delivered=0, pending=total) and len(none) == 0
        assert np.array_equal(p.read_watch(), WM.fresh(G))
        # the device form at a cut inside the second wave, then the rest with room to spare
        cut = 70
        buf = torch.full(((n + 1) * 6,), -7, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        first = d.poll_leaders_dev(buf.data_ptr(), cut, g0, n)
        assert first == dict(info, delivered=cut, pending=total - cut)
        raw = buf.cpu().numpy()
        same(raw[:cut * 6].view(abi.EVENT_DTYPE), ev[:cut], "device events, first poll")
        assert (raw[cut * 6:] == -7).all()
        buf.fill_(-7)
        torch.cuda.synchronize()
        rest = d.poll_leaders_dev(buf.data_ptr(), n, g0, n)
        assert rest["delivered"] == total - cut and rest["pending"] == 0
        raw = buf.cpu().numpy()
        same(raw[:(total - cut) * 6].view(abi.EVENT_DTYPE), ev[cut:], "device events, second poll")
        assert (raw[(total - cut) * 6:] == -7).all()
        assert np.array_equal(a.read_watch(), d.read_watch())
        # a peek through the device form: no buffer at all
        assert d.poll_leaders_dev(0, 0, g0, n) == dict.fromkeys(abi.WATCH_INFO_FIELDS, 0) | \
            {"leaderless": info["leaderless"]}
        with pytest.raises(ValueError, match="8-byte"):
            d.poll_leaders_dev(buf.data_ptr() + 4, 4, g0, n)
        wi = abi.raft_watch_info()
        assert d._lib.raft_engine_poll_leaders_dev(d._h, 0, G, C.c_void_p(buf.data_ptr() + 4), 4, C.byref(wi)) == \
            abi.RAFT_EINVAL and b"8-byte" in d._lib.raft_last_error()
        assert (buf.cpu().numpy() == raw).all()
        assert a.digest() == d.digest() == p.digest() == dg


def test_crafted_groups_on_the_device():
    """watch_model.crafted() and crafted_single() written with write_state and
    write_watch: the events and info written out by hand."""
    for w, seen, R, want_ev, want_info, want_seen in (
            (*WM.crafted(), WM.CR, WM.CRAFTED_EVENTS, WM.CRAFTED_INFO, WM.CRAFTED_SEEN_AFTER),
            (*WM.crafted_single(), 1, WM.CRAFTED_SINGLE_EVENTS, WM.CRAFTED_SINGLE_INFO, None)):
        with RaftEngine(abi.make_params(R=R, G=len(w), log_cap=8)) as e:
            e.write_state(w)
            e.write_watch(seen)
            assert np.array_equal(e.read_watch(), seen)
            dg = e.digest()
            info, ev = e.poll_leaders()
            assert info == want_info
            same(ev, want_ev, f"crafted events (R {R})")
            if want_seen is not None:
                assert np.array_equal(e.read_watch(), want_seen)
            again, none = e.poll_leaders()
            assert len(none) == 0 and again == dict(dict.fromkeys(abi.WATCH_INFO_FIELDS, 0),
                                                    leaderless=want_info["leaderless"])
            assert e.digest() == dg


def test_write_watch_resumes_and_reset_starts_over():
    """A second engine brought to the first one's state and watch reports what
    the first reports next; raft_engine_reset puts the watch back to (-1, 0);
    trim_staging keeps it; a bad pair is refused with nothing stored."""
    R, G = 5, 203
    kw = WM.parity_kw(R, G, "flat")
    with RaftEngine(abi.make_params(**kw)) as a, RaftEngine(abi.make_params(**kw)) as b:
        for e in (a, b):
            e.step(WM.WARM_STEPS, counters=False)
        _, first = a.poll_leaders()
        assert len(first) >= 66
        b.write_watch(a.read_watch())
        for e in (a, b):
            e.step(WM.RUN_ON_STEPS, counters=False)
        a.trim_staging()
        ia, ea = a.poll_leaders()
        ib, eb = b.poll_leaders()
        assert ia == ib and 0 < len(ea) < G and (ea["prev_leader"] >= 0).any()
        same(ea, eb, "resumed events")
        assert np.array_equal(a.read_watch(), b.read_watch())
        # refused pairs: through the library itself, nothing stored
        before = b.read_watch()
        for pair in ((R, 1), (-2, 0), (0, -1), (-1, 3)):
            bad = before.copy()
            bad[G - 1] = pair
            assert b._lib.raft_engine_write_watch(b._h, 0, G, abi.ptr(bad, C.c_int32)) == abi.RAFT_EINVAL
            assert np.array_equal(b.read_watch(), before)
        bytes_before = a.device_bytes
        a.reset()
        assert np.array_equal(a.read_watch(), WM.fresh(G)) and a.device_bytes == bytes_before
        a.step(WM.WARM_STEPS, counters=False)
        _, again = a.poll_leaders()
        same(again, first, "the first poll after a reset")


def test_error_paths():
    """Null info, a negative max_events, a null buffer with room, groups outside
    the engine: refused with a zeroed info and nothing stored; n == 0 is RAFT_OK."""
    R, G = 5, 70
    with RaftEngine(abi.make_params(R=R, G=G, seed=11, log_cap=64, cmd_ppm=100_000)) as e:
        e.step(WM.WARM_STEPS, counters=False)
        lib, h = e._lib, e._h
        st, seen = e.read_state(), e.read_watch()
        buf = np.zeros(G, abi.EVENT_DTYPE)
        p = C.c_void_p(buf.ctypes.data)
        info = abi.raft_watch_info()
        for fn in (lib.raft_engine_poll_leaders, lib.raft_engine_poll_leaders_dev):
            assert fn(h, 0, G, p, G, None) == abi.RAFT_EINVAL and b"null info" in lib.raft_last_error()
            for g0, n, room in ((G, 1, 4), (-1, 2, 4), (G - 1, 2, 4), (0, -1, 4), (0, G, -1), (G, 0, 4), (3, 0, 0)):
                info.pending = info.leaderless = 5
                want = WM.poll(st, seen.copy(), R, g0, n, room)[2]
                assert fn(h, g0, n, p, room, C.byref(info)) == want, (g0, n, room)
                assert info.pending == 0 and info.leaderless == 0
            info.pending = 5
            assert fn(h, 0, G, None, 4, C.byref(info)) == abi.RAFT_EINVAL and info.pending == 0
            assert b"null record buffer" in lib.raft_last_error()
        assert np.array_equal(e.read_watch(), seen) and not buf.view(np.int32).any()
        with pytest.raises(RaftError, match="outside the engine"):
            e.poll_leaders(G - 1, 2)
        with pytest.raises(RaftError, match="outside the engine"):
            e.read_watch(G - 1, 2)
        info_, ev = e.poll_leaders(5, 0)
        assert info_ == dict.fromkeys(abi.WATCH_INFO_FIELDS, 0) and len(ev) == 0 and ev.dtype == abi.EVENT_DTYPE
        # the host buffer is written to the end of its records and not beyond
        raw = np.full((G + 1) * 6, -7, np.int32)
        assert lib.raft_engine_poll_leaders(h, 0, G, C.c_void_p(raw.ctypes.data), G, C.byref(info)) == abi.RAFT_OK
        assert 0 < info.delivered <= G and (raw[info.delivered * 6:] == -7).all()
        assert (raw[:info.delivered * 6].view(abi.EVENT_DTYPE)["prev_leader"] == -1).all()


def test_the_service_keeps_a_leader_directory():
    """RaftService.watch_leaders over a faulted run: after each poll the cached
    directory equals the one computed from read_state, newest_leader reads it,
    and RaftService.leader is what it was."""
    R, G = 5, 203
    with RaftEngine(abi.make_params(**WM.parity_kw(R, G, "textbook"))) as e:
        svc = service.RaftService(e)
        assert svc.newest_leader(7) is None
        sizes = []
        for steps in (WM.WARM_STEPS, WM.SETTLE_STEPS, WM.RUN_ON_STEPS, 1):
            e.step(steps, counters=False)
            ev = svc.watch_leaders()
            sizes.append(len(ev))
            st = e.read_state()
            leader, term = WM.directory(st, R)
            assert np.array_equal(svc.leader_of, leader) and np.array_equal(svc.term_of, term)
            assert svc.last_watch["delivered"] == len(ev) and svc.last_watch["pending"] == 0
        assert sizes[0] >= 66 and 0 < sizes[1] < sizes[0] and 0 < sizes[2]
        led = int(np.nonzero(leader >= 0)[0][0])
        node = svc.newest_leader(led)
        assert (node.group, node.replica) == (led, int(leader[led])) and node.state == "LEADER"
        assert svc.newest_leader(int(np.nonzero(leader < 0)[0][0])) is None
        # a deposed leader at a lower index: leader() names it, newest_leader() its successor
        lowest = e.leaders()["leader"]
        split = np.nonzero(lowest != leader)[0]
        if len(split):
            g = int(split[0])
            assert svc.leader(g).replica == int(lowest[g]) < svc.newest_leader(g).replica
        # a bounded poll leaves the rest pending and the directory partly updated
        e.step(WM.RUN_ON_STEPS, counters=False)
        ev = svc.watch_leaders(max_events=3)
        assert len(ev) == 3 and svc.last_watch["pending"] > 0
        svc.watch_leaders()
        leader, term = WM.directory(e.read_state(), R)
        assert np.array_equal(svc.leader_of, leader) and np.array_equal(svc.term_of, term)
