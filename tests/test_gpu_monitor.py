"""The liveness monitor on the GPU (marker `gpu`): raft_monitor_* against
tests/monitor_model.py over the engine's own exported state.  Every comparison
is exact: the info of every observe, the ledger (raft_monitor_read), the full
`now` and `ever` reports and the availability totals."""
import ctypes as C
import importlib

import numpy as np
import pytest

import client_model as CM
import monitor_model as MM
import noop_model as NM
import restart_model as RM
from helpers import abi, fld

pytestmark = pytest.mark.gpu

eng_mod = importlib.import_module("raft-kotlin_amd.engine")
service = importlib.import_module("raft-kotlin_amd.service")
RaftEngine = eng_mod.RaftEngine
RaftError = eng_mod.RaftError
EV_WORDS = abi.MONITOR_EVENT_DTYPE.itemsize // 4


def same(got, want, label=""):
    assert got.dtype == want.dtype and len(got) == len(want), (label, got.dtype, len(got), len(want))
    if not np.array_equal(got, want):
        at = int(np.nonzero(got != want)[0][0])
        raise AssertionError(f"{label}: {int((got != want).sum())} records differ; first at {at}: {got[at]} vs {want[at]}")


def same_ledger(got, want, label=""):
    if not np.array_equal(got, want):
        g, w = np.argwhere(got != want)[0]
        raise AssertionError(f"{label}: {int((got != want).any(axis=1).sum())} ledgers differ; first group {g} word "
                             f"{abi.MONITOR_WORD_NAMES[w]}: {got[g]} vs {want[g]}")


class Shadow:
    """A RaftEngine with a monitor whose every observe is checked, as it
    happens, against the model over the engine's own exported state and a
    ledger and totals carried here: the info, raft_monitor_read, the full now
    and ever reports and the availability totals."""

    def __init__(self, e, cfg, ledger=None, avail=None):
        self.e, self.cfg, self.m = e, cfg, e.monitor(**cfg)
        self.ledger = MM.fresh(e.G) if ledger is None else ledger.copy()
        self.avail = MM.zero_avail() if avail is None else {k: np.copy(v) if k == "hist" else v for k, v in avail.items()}
        if ledger is not None:
            self.m.write(ledger)
        if avail is not None:
            self.m.set_availability(**avail)

    def observe(self, g0=0, n=None, label=""):
        e = self.e
        want, rc = MM.observe(e.read_state(), self.ledger, self.avail, self.cfg, e.R, e.cap, e.step_index, g0, n)
        assert rc == abi.RAFT_OK
        got = self.m.observe(g0, n)
        assert got == want, (label, got, want)
        self.check(label)
        return got

    def check(self, label=""):
        same_ledger(self.m.read(), self.ledger, label)
        for ever in (False, True):
            winfo, wev, _ = MM.report(self.ledger, ever=ever)
            info, ev = self.m.report(ever=ever)
            assert info == winfo, (label, ever, info, winfo)
            same(ev, wev, f"{label}: report ever={ever}")
        av = self.m.availability()
        assert MM.same_avail(av, self.avail), (label, av, self.avail)


def test_crafted_groups_on_the_device():
    """monitor_model.CRAFTED through write_state with the step index set per
    phase: the now and ever words written out by hand after each phase, the
    ledger, info and totals the model's; a second monitor resumed after phase 0
    (raft_monitor_write, raft_monitor_set_availability) ends identical; the host
    and _dev report forms agree and a sentinel past the last record is intact."""
    import torch
    names = MM.CRAFTED_NAMES
    with RaftEngine(abi.make_params(R=MM.CR, G=len(names), log_cap=MM.CCAP)) as e:
        s = Shadow(e, MM.CRAFTED_CFG, MM.crafted_ledger0())
        for k in range(3):
            e.write_state(MM.crafted_phase(k))
            e.step_index = MM.CRAFTED_STEPS[k]
            dg = e.digest()
            s.observe(label=f"phase {k}")
            assert e.digest() == dg
            L = s.m.read()
            assert np.array_equal(L[:, MM.NOW], MM.crafted_now(k)) and np.array_equal(L[:, MM.EVER], MM.crafted_ever(k))
            if k == 0:
                r = Shadow(e, MM.CRAFTED_CFG, s.ledger, s.avail)           # resumed from here on
            else:
                r.observe(label=f"resumed, phase {k}")
        same_ledger(r.m.read(), s.m.read(), "resumed")
        assert MM.same_avail(r.m.availability(), s.m.availability()) and MM.same_avail(s.avail, MM.crafted_avail())
        for name, words in MM.CRAFTED_WORDS.items():
            row = L[names.index(name)]
            assert {w: int(row[w]) for w in words} == words, name
        # the _dev form: the same records, nothing beyond them
        for ever in (False, True):
            info, ev = s.m.report(ever=ever)
            assert len(ev) == int((MM.crafted_ever(2) if ever else MM.crafted_now(2)).astype(bool).sum()) > 0
            buf = torch.full(((len(names) + 1) * EV_WORDS,), -7, dtype=torch.int32, device="cuda:0")
            torch.cuda.synchronize()
            assert s.m.report_dev(buf.data_ptr(), len(names), ever=ever) == info
            raw = buf.cpu().numpy()
            same(raw[:len(ev) * EV_WORDS].view(abi.MONITOR_EVENT_DTYPE), ev, "device events")
            assert (raw[len(ev) * EV_WORDS:] == -7).all()


PARITY = [(R, mode, W) for R in (3, 5, 8) for mode in ("reference", "textbook") for W in (0, 16)]
PARITY_CFG = MM.config(leaderless_steps=2, stalled_steps=5, lag_entries=6, churn_terms=2, churn_steps=15)
PARITY_GAPS = [1, 3, 7, 20] * 3 + [20, 7]


@pytest.mark.parametrize("R,mode,W", PARITY, ids=[f"R{r}-{m}-{'ring' if w else 'flat'}" for r, m, w in PARITY])
def test_parity_after_every_observe(R, mode, W):
    """G = 203 under drops, churn, partitions and commands, with persistent
    restart_random between launches: after every observe -- 1, 3, 7 and 20 steps
    apart, 120 steps in all, whole engine and a sub-range -- the info, the
    ledger, both reports and the totals equal the model's."""
    assert sum(PARITY_GAPS) == 120
    kw = dict(R=R, G=203, seed=11, log_cap=300, log_window=W, **RM.STRESS_MIX)
    if mode == "textbook":
        kw.update(mode=abi.MODE_TEXTBOOK, ae_max_entries=4)
    with RaftEngine(abi.make_params(**kw)) as e:
        s = Shadow(e, PARITY_CFG)
        s.observe(label="fresh")
        seen = MM.zero_info()
        for k, gap in enumerate(PARITY_GAPS):
            if k in (5, 9):
                e.restart(ppm=150_000, down_steps=4)
            e.step(gap, counters=False)
            info = s.observe(label=f"step {e.step_index}") if k != 6 else s.observe(5, 100, label="groups [5, 105)")
            for key in seen:
                seen[key] += info[key]
        assert e.step_index == 120
        assert seen["outages_ended"] > 0 and seen["leaderless"] > 0 and seen["cleared"] > 0 and seen["lagging"] > 0
        assert s.avail["outages"] == seen["outages_ended"] and (s.ledger[:, MM.LEADER] >= 0).any()


def test_counter_identity_on_the_engine():
    """G = 203, 60 faulted steps, one observe per step with leaderless_steps = 0:
    info.leaderless is G - RAFT_C_GROUPS_WITH_LEADER of the engine's own counter
    row; at the end the ended outages' lengths plus the running ones' (their
    ages one step on, test_monitor_cpu.py says why) add up to the group-steps
    without a leader, and the histogram counts every ended outage."""
    G, steps = 203, 60
    with RaftEngine(abi.make_params(**RM.parity_kw(5, G, "flat"))) as e:
        m = e.monitor(leaderless_steps=0)
        without = []
        for t in range(1, steps + 1):
            row = e.step(1)[-1]
            info = m.observe()
            without.append(G - int(row[abi.C_INDEX["groups_with_leader"]]))
            assert info["leaderless"] == info["down"] == without[-1], (t, info, without[-1])
        L, av = m.read(), m.availability()
        running = L[:, MM.DOWN_SINCE] != -1
        so_far = int(MM.age(steps + 1, L[running, MM.DOWN_SINCE].astype(np.int64)).sum())
        assert int(L[:, MM.DOWN_TOTAL].sum()) + so_far == sum(without)
        assert int(av["hist"].sum()) == int(L[:, MM.OUTAGES].sum()) == av["outages"] > 0
        assert av["down_steps"] == int(L[:, MM.DOWN_TOTAL].sum())


def test_observe_and_report_never_write_the_engine():
    """raft_engine_digest, read_state, read_applied and read_watch are equal
    before and after observe + report (host, peek and filtered forms)."""
    with RaftEngine(abi.make_params(**RM.parity_kw(5, 203, "flat"))) as e:
        e.step(40, counters=False)
        e.drain_committed()
        e.poll_leaders()
        m = e.monitor(leaderless_steps=0, stalled_steps=0, lag_entries=1, churn_terms=1, churn_steps=5)
        snap = lambda: (e.digest(), e.read_state(), e.applied(), e.read_watch())
        before = snap()
        info = m.observe()
        assert info["flagged"] > 0
        m.report()
        m.report(max_events=0)
        m.report(ever=True, kinds=abi.MONITOR_LAGGING)
        m.availability()
        after = snap()
        assert before[0] == after[0] and all(np.array_equal(x, y) for x, y in zip(before[1:], after[1:]))
        m.close()


def tiled(k: int, G: int) -> np.ndarray:
    """Phase k of the crafted groups, repeated to G groups."""
    one = MM.crafted_phase(k)
    return np.tile(one, (-(-G // len(one)), 1))[:G]


def test_sub_ranges_and_report_cuts():
    """Observes with g0 > 0 and n no multiple of 8, 32 or 64 touch only their
    groups; report cuts at 0 (a peek: pending equals the total), 1, the middle,
    exactly the total and beyond, on a sub-range, host and _dev forms; the kinds
    filter; now against ever after groups cleared."""
    import torch
    G = 203
    with RaftEngine(abi.make_params(R=MM.CR, G=G, log_cap=MM.CCAP)) as e:
        s = Shadow(e, MM.CRAFTED_CFG)
        for k in range(2):
            e.write_state(tiled(k, G))
            e.step_index = MM.CRAFTED_STEPS[k]
            s.observe(label=f"phase {k}")
        e.write_state(tiled(2, G))
        e.step_index = MM.CRAFTED_STEPS[2]
        before = s.m.read()
        s.observe(9, 83, label="groups [9, 92)")
        L = s.m.read()
        outside = np.ones(G, bool)
        outside[9:92] = False
        same_ledger(L[outside], before[outside], "outside the range")
        assert (L[9:92] != before[9:92]).any()
        s.observe(101, 97, label="groups [101, 198)")
        g0, n = 5, 150
        _, whole, _ = MM.report(s.ledger, g0, n, ever=True)
        total = len(whole)
        assert total > 8
        buf = torch.full(((total + 6) * EV_WORDS,), -7, dtype=torch.int32, device="cuda:0")
        for cut in (0, 1, total // 2, total, total + 5):
            winfo, wev, _ = MM.report(s.ledger, g0, n, cut, ever=True)
            info, ev = s.m.report(g0, n, cut, ever=True)
            assert info == winfo and info["pending"] == total - min(cut, total)
            same(ev, wev, f"cut {cut}")
            buf.fill_(-7)
            torch.cuda.synchronize()
            assert s.m.report_dev(buf.data_ptr() if cut else 0, cut, g0, n, ever=True) == winfo
            raw = buf.cpu().numpy()
            same(raw[:len(wev) * EV_WORDS].view(abi.MONITOR_EVENT_DTYPE), wev, f"device cut {cut}")
            assert (raw[len(wev) * EV_WORDS:] == -7).all()
        for ever in (False, True):
            for kinds in (MM.LL, MM.ST, MM.LAG, MM.CH, MM.ST | MM.CH, 0):
                winfo, wev, _ = MM.report(s.ledger, 3, 190, ever=ever, kinds=kinds)
                info, ev = s.m.report(3, 190, ever=ever, kinds=kinds)
                assert info == winfo and (not ever or (len(wev) > 0) == (kinds != 0)), (ever, kinds)
                same(ev, wev, f"kinds {kinds} ever={ever}")
        now, ever = s.m.report()[1], s.m.report(ever=True)[1]
        gone = np.setdiff1d(ever["group"], now["group"])
        assert len(gone) > 0 and (s.ledger[gone, MM.NOW] == 0).all() and (s.ledger[gone, MM.EVER] != 0).all()
        same_ledger(s.m.read(), s.ledger, "a report consumes nothing")


def test_past_one_workgroup_a_partial_last_wave_and_one_scan_block():
    """G = 300,001, R = 3: states built in numpy and loaded with write_state,
    never stepped; about every 100th group shows each bit at the second
    observe.  Info, ledger, reports and totals are the model's.  The size is
    past one workgroup, ends in a partial wave, and gives the report's stream
    4,688 wave counts to scan: more than one block of rocprim's scan, which
    takes 256 x 8 = 2,048 eight-byte items per block by default and 256 x 15 =
    3,840 in its tuned gfx942 configuration (131,072 and 245,760 groups; G =
    70,001 would stay inside one).  The order of the 32-byte records across the
    block boundary, and a cut inside the last block, are checked."""
    G = 300_001
    assert (G + 63) // 64 > 256 * 15
    p0, p1, want = MM.bulk(G)
    with RaftEngine(abi.make_params(R=3, G=G, log_cap=16)) as e:
        s = Shadow(e, MM.BULK_CFG)
        e.write_state(p0)
        e.step_index = MM.BULK_STEPS[0]
        first = s.observe(label="phase 0")
        assert first["flagged"] == 0 and first["down"] == len(range(10, G, 100)) == 3000
        e.write_state(p1)
        e.step_index = MM.BULK_STEPS[1]
        info = s.observe(label="phase 1")
        assert np.array_equal(s.m.read()[:, MM.NOW], want)
        assert info["flagged"] == info["newly_flagged"] == int((want != 0).sum()) == 15000
        assert [info[k] for k in abi.MONITOR_KINDS] == [3000, 6000, 6000, 6000]
        _, ev = s.m.report()
        assert (np.diff(ev["group"]) > 0).all() and ev["group"][0] == 10 and ev["group"][-1] == 299_938
        assert (ev["group"] < 64 * 2048).any() and (ev["group"] >= 64 * 3840).any()   # records on both sides of a block
        for cut in (14_993, 12_000):                                    # in the last scan block, and further down
            winfo, wev, _ = MM.report(s.ledger, 0, G, cut)
            cinfo, cev = s.m.report(max_events=cut)
            assert cinfo == winfo and cinfo["pending"] == 15000 - cut
            same(cev, wev, f"cut {cut}")
        # a steady observe stores nothing and reports the same
        again = s.observe(label="steady")
        assert again == dict(info, newly_flagged=0)


def test_refusals_and_device_bytes():
    """The refusals of include/raft_engine.h: a null handle, info or config, a
    bad config, a negative max_events, a null buffer with room, a misaligned
    _dev buffer, another `which`, unknown kinds (RAFT_EINVAL), groups outside the
    engine (RAFT_ERANGE), n == 0 (RAFT_OK, zeroed info); a refused
    raft_monitor_write or _set_availability stores nothing; the ledger counts in
    raft_monitor_device_bytes and not in raft_engine_device_bytes;
    raft_engine_reset does not reach the monitor."""
    import torch
    R, G, cap = 5, 70, 64
    with RaftEngine(abi.make_params(R=R, G=G, seed=11, log_cap=cap, cmd_ppm=100_000, drop_ppm=100_000)) as e:
        before = e.device_bytes
        m = e.monitor(leaderless_steps=0, stalled_steps=1, lag_entries=1)
        assert m.device_bytes == ((64 * G + 255) & ~255) + 512 and e.device_bytes == before
        assert m.observe()["down"] == G                                 # the wait for the first leader begins
        e.step(40, counters=False)
        m.observe()
        lib, h = e._lib, m._h
        L, av = m.read(), m.availability()
        assert av["outages"] > 0
        mi, ri = abi.raft_monitor_info(), abi.raft_monitor_report_info()
        buf = np.zeros(G, abi.MONITOR_EVENT_DTYPE)
        p = C.c_void_p(buf.ctypes.data)
        dev = torch.zeros(G * EV_WORDS + 8, dtype=torch.int32, device="cuda:0")
        assert lib.raft_monitor_observe(None, 0, G, C.byref(mi)) == abi.RAFT_EINVAL
        assert lib.raft_monitor_observe(h, 0, G, None) == abi.RAFT_EINVAL and b"null info" in lib.raft_last_error()
        cfg, out = abi.raft_monitor_config(), C.c_void_p()
        assert lib.raft_monitor_create(None, C.byref(cfg), C.byref(out)) == abi.RAFT_EINVAL
        assert lib.raft_monitor_create(e._h, None, C.byref(out)) == abi.RAFT_EINVAL
        assert lib.raft_monitor_create(e._h, C.byref(cfg), None) == abi.RAFT_EINVAL
        for kw in (dict(leaderless_steps=-1), dict(stalled_steps=-1), dict(lag_entries=-1), dict(churn_terms=-1),
                   dict(churn_steps=-1), dict(churn_terms=1, churn_steps=0)):
            assert not MM.valid_config(MM.config(**kw))
            bad = abi.raft_monitor_config(**kw)
            assert lib.raft_monitor_create(e._h, C.byref(bad), C.byref(out)) == abi.RAFT_EINVAL and not out.value, kw
        bad = abi.raft_monitor_config()
        bad.reserved[1] = 1
        assert lib.raft_monitor_create(e._h, C.byref(bad), C.byref(out)) == abi.RAFT_EINVAL and not out.value
        assert lib.raft_monitor_destroy(None) == abi.RAFT_OK and lib.raft_monitor_reset(None) == abi.RAFT_EINVAL
        assert lib.raft_monitor_device_bytes(None) == 0
        for g0, n in ((G, 1), (-1, 2), (G - 1, 2), (0, -1)):
            mi.flagged = mi.down = 5
            assert lib.raft_monitor_observe(h, g0, n, C.byref(mi)) == abi.RAFT_ERANGE
            assert mi.flagged == 0 and mi.down == 0
            assert lib.raft_monitor_read(h, g0, n, abi.ptr(L, C.c_int32)) == abi.RAFT_ERANGE
        for g0 in (G, 3):
            mi.flagged = 5
            assert lib.raft_monitor_observe(h, g0, 0, C.byref(mi)) == abi.RAFT_OK and mi.flagged == 0
        NOW, ALL = abi.MONITOR_NOW, abi.MONITOR_ALL
        for fn, ptr in ((lib.raft_monitor_report, p), (lib.raft_monitor_report_dev, C.c_void_p(dev.data_ptr()))):
            assert fn(None, 0, G, NOW, ALL, ptr, G, C.byref(ri)) == abi.RAFT_EINVAL
            assert fn(h, 0, G, NOW, ALL, ptr, G, None) == abi.RAFT_EINVAL
            for g0, n, which, kinds, room, rc in (
                    (G, 1, NOW, ALL, 4, abi.RAFT_ERANGE), (0, G + 1, NOW, ALL, 4, abi.RAFT_ERANGE),
                    (0, G, NOW, ALL, -1, abi.RAFT_EINVAL), (0, G, 2, ALL, 4, abi.RAFT_EINVAL),
                    (0, G, -1, ALL, 4, abi.RAFT_EINVAL), (0, G, NOW, 16, 4, abi.RAFT_EINVAL),
                    (0, G, NOW, -1, 4, abi.RAFT_EINVAL), (G, 0, NOW, ALL, 4, abi.RAFT_OK), (3, 0, 1, 0, 0, abi.RAFT_OK)):
                ri.pending = ri.flagged = 5
                assert fn(h, g0, n, which, kinds, ptr, room, C.byref(ri)) == rc, (g0, n, which, kinds, room)
                assert ri.pending == 0 and ri.flagged == 0
            ri.pending = 5
            assert fn(h, 0, G, NOW, ALL, None, 4, C.byref(ri)) == abi.RAFT_EINVAL and ri.pending == 0
            assert b"null record buffer" in lib.raft_last_error()
        assert lib.raft_monitor_report_dev(h, 0, G, NOW, ALL, C.c_void_p(dev.data_ptr() + 8), 4, C.byref(ri)) == abi.RAFT_EINVAL
        assert b"16-byte" in lib.raft_last_error()
        with pytest.raises(ValueError, match="16-byte"):
            m.report_dev(dev.data_ptr() + 8, 4)
        with pytest.raises(ValueError, match="kinds"):
            m.report(kinds=16)
        assert not buf.view(np.int32).any() and not dev.cpu().numpy().any()
        # refused ledgers: through the library itself, nothing stored
        for word, v in ((MM.NOW, 16), (MM.NOW, -1), (MM.EVER, 32), (MM.LEADER, R), (MM.LEADER, -2), (MM.LAG_MASK, 1 << R),
                        (MM.LAG_MASK, -1), (MM.OUTAGES, -1), (MM.DOWN_TOTAL, -1), (MM.LONGEST, -5), (MM.MAX_LAG, -1),
                        (MM.STALL_MARK, -1), (MM.RSV0, 1), (MM.RSV1, -1)):
            bad = L.copy()
            bad[:, MM.FIRST] += 1                                       # (would be stored in every group if accepted)
            bad[G - 1, word] = v
            assert not MM.valid_ledger(bad, R)
            assert lib.raft_monitor_write(h, 0, G, abi.ptr(bad, C.c_int32)) == abi.RAFT_EINVAL, (word, v)
            same_ledger(m.read(), L, "after a refused write")
        assert lib.raft_monitor_write(h, 0, G, None) == abi.RAFT_EINVAL
        for k in (0, 31, 32, 33, 34, 35):
            raw = abi.raft_monitor_availability()
            C.cast(C.pointer(raw), C.POINTER(C.c_int64))[k] = -1 if k < 34 else 1
            assert lib.raft_monitor_set_availability(h, C.byref(raw)) == abi.RAFT_EINVAL, k
        assert lib.raft_monitor_set_availability(h, None) == abi.RAFT_EINVAL
        assert lib.raft_monitor_get_availability(h, None) == abi.RAFT_EINVAL
        assert MM.same_avail(m.availability(), av)
        # the edges of what a write accepts: no word of them is an index
        edge = L.copy()
        edge[0, MM.NOW], edge[0, MM.EVER], edge[0, MM.LEADER], edge[0, MM.LAG_MASK] = 15, 15, R - 1, (1 << R) - 1
        edge[0, [MM.FIRST, MM.DOWN_SINCE, MM.STALL_SINCE, MM.WIN_START, MM.WIN_TERM]] = -7
        edge[0, [MM.OUTAGES, MM.DOWN_TOTAL, MM.LONGEST, MM.MAX_LAG, MM.STALL_MARK]] = 2 ** 31 - 1
        edge[1, MM.DOWN_SINCE], edge[1, MM.STALL_SINCE] = 2 ** 31 - 1, -2 ** 31
        m.write(edge)
        same_ledger(m.read(), edge, "the edges of what a write accepts")
        want, wav = edge.copy(), {k: np.copy(v) if k == "hist" else v for k, v in av.items()}
        winfo, _ = MM.observe(e.read_state(), want, wav, m.config, R, cap, e.step_index)
        assert m.observe() == winfo
        same_ledger(m.read(), want, "observed from the edge ledger")
        assert MM.same_avail(m.availability(), wav)
        with pytest.raises(RaftError, match="outside the engine"):
            m.observe(G - 1, 2)
        # raft_engine_reset does not reach the monitor; raft_monitor_reset equals a fresh handle
        e.reset()
        same_ledger(m.read(), want, "after raft_engine_reset")
        assert MM.same_avail(m.availability(), wav)
        m.reset()
        same_ledger(m.read(), MM.fresh(G), "reset")
        assert MM.same_avail(m.availability(), MM.zero_avail())
        assert m.report(ever=True)[0] == dict(delivered=0, pending=0, flagged=0)
        m.close()
        m.close()


def test_the_remedy_loop_end_to_end():
    """The stalled commit of Raft thesis 3.6.2 on an idle textbook engine
    (noop_model.LIVE_KW), found and healed through the service.  Once every
    group has a leader a command is proposed to every group; one step later
    (the entry is on every replica, committed on the old leader) replica 0 is
    evacuated.  The groups it led get a leader of a higher term whose log ends
    with that entry of the earlier term, above its own commit point: idle, it
    never commits it.  (noop_model.stalled_tickets itself evacuates with no step
    in between: the entry then exists on the deposed leader alone, the new
    leader's log is empty, and by rule 2 -- lastIndex_L > hi_L -- there is no
    backlog to flag; its tickets end LOST, not committed.)  check_liveness with
    stalled_steps = 10 flags, after 10 more steps, exactly the groups the model
    says -- the groups replica 0 led; remediate() appends their no-ops; a few
    steps later an observe reports them cleared, `ever` still names them and
    unavailable() is empty."""
    with RaftEngine(abi.make_params(**NM.LIVE_KW)) as e:
        G, R = e.G, e.R
        svc = service.RaftService(e)
        assert len(svc.unavailable()) == 0 and svc.remediate() == {"noops": None, "install": None}
        groups = np.arange(G, dtype=np.int64)
        NM.step_until(e, NM.all_led(e))
        led0 = np.nonzero(e.leaders()["leader"] == 0)[0]
        assert 0 < len(led0) < G
        cmds = (1000 + groups).astype(np.uint32)
        tk = e.propose(groups, cmds)
        e.step(1, counters=False)
        e.evacuate(np.full(G, 1, np.uint8))
        for _ in range(NM.STEP_LIMIT):
            e.step(1, counters=False)
            st = e.read_state()
            term = np.stack([fld(st, R, r, "term") for r in range(R)], 1)
            lead = np.stack([fld(st, R, r, "role") == abi.LEADER for r in range(R)], 1)
            if (np.where(lead, term, -1).max(axis=1)[led0] > tk["term"][led0]).all():
                break
        e.step(30, counters=False)
        cfg = MM.config(leaderless_steps=3, stalled_steps=10)
        svc.liveness_monitor = e.monitor(**cfg)
        ledger, avail = MM.fresh(G), MM.zero_avail()
        model = lambda: MM.observe(e.read_state(), ledger, avail, cfg, R, e.cap, e.step_index)[0]
        assert svc.check_liveness() == model()
        assert svc.last_liveness[0]["flagged"] == 0 and len(svc.unavailable()) == 0
        e.step(10, counters=False)
        info = svc.check_liveness()
        assert info == model()
        ev = svc.unavailable()
        assert ev.dtype == abi.MONITOR_EVENT_DTYPE and np.array_equal(ev["group"], np.nonzero(ledger[:, MM.NOW])[0])
        assert np.array_equal(ev["group"], led0) and (ev["now"] == abi.MONITOR_COMMIT_STALLED).all()
        assert info["commit_stalled"] == info["flagged"] == info["newly_flagged"] == len(led0)
        assert len(svc.unavailable(kinds=abi.MONITOR_LEADERLESS)) == 0 and len(svc.unavailable(max_events=1)) == 1
        t0, dg = e.step_index, e.digest()
        fix = svc.remediate()
        assert e.step_index == t0 and e.digest() != dg                  # never stepped; the no-ops were written
        assert fix["install"] is None and fix["noops"]["appended"] == len(led0)
        assert fix["noops"]["current"] + fix["noops"]["appended"] == G
        e.step(6, counters=False)                                       # the no-ops commit, and the entries below them
        assert (e.resolve(groups, tk, cmds)["status"] == CM.COMMITTED).all()
        info = svc.check_liveness()
        assert info == model()
        assert info["cleared"] == len(led0) and info["flagged"] == 0
        assert len(svc.unavailable()) == 0
        _, ever = svc.liveness_monitor.report(ever=True)
        assert np.array_equal(ever["group"], led0) and (ever["ever"] == abi.MONITOR_COMMIT_STALLED).all()
        assert (ever["now"] == 0).all() and (ever["stall_since"] == -1).all()


def test_the_remedy_loop_heals_lagging_replicas():
    """remediate()'s other branch, against snapshot_model's Host driven through
    the same calls: reference mode, R = 5, G = 203 under drops, churn, partitions
    and commands, the machine configured, replicas restarted with ten down-steps
    so that some fall behind.  check_liveness with lag_entries = 6 counts the
    groups the model says; remediate() runs apply_committed and
    install_snapshot(min_lag = 6) over the observed range -- their infos, the
    state, the logs and the digest afterwards equal the Host's -- and appends no
    no-op in reference mode; the next observe, with no step in between, reports
    the healed groups cleared and only replicas ahead of their leader's term
    still lag."""
    import snapshot_model as SM
    from helpers import assert_same_logs, assert_same_state
    kw, lag = RM.parity_kw(5, 203, "flat"), 6
    cfg = MM.config(leaderless_steps=1000, stalled_steps=0, lag_entries=lag)
    h = SM.Host(8, **kw)
    with RaftEngine(abi.make_params(**kw)) as e:
        e.sm_configure(8)
        svc = service.RaftService(e)
        svc.liveness_monitor = e.monitor(**cfg)
        for x in (e, h):
            x.step(40)
            x.restart(ppm=150_000, down_steps=10)
            x.step(30)
        ledger, avail = MM.fresh(e.G), MM.zero_avail()
        model = lambda: MM.observe(e.read_state(), ledger, avail, cfg, e.R, e.cap, e.step_index)[0]
        before = svc.check_liveness()
        assert before == model() and before["lagging"] > 20 and before["commit_stalled"] > 0
        want_apply, want_install = h.sm_apply(), h.install_snapshot(min_lag=lag)
        t0 = e.step_index
        fix = svc.remediate()
        assert e.step_index == t0 and fix["noops"] is None              # reference mode: no no-ops, whatever stalled
        assert svc.last_heal_apply == want_apply and fix["install"] == want_install, (fix, want_install)
        assert fix["install"]["installed"] > 0 and fix["install"]["ahead"] > 0
        assert_same_state(e.read_state(), h.read_state(), e.R, "after the install")
        assert_same_logs(e.read_state(), e.read_log(), h.read_log(), e.R, "after the install")
        assert e.digest() == h.digest()
        after = svc.check_liveness()
        assert after == model()
        assert 0 < after["lagging"] <= fix["install"]["ahead"] and after["lagging"] < before["lagging"]
        left = svc.unavailable(kinds=abi.MONITOR_LAGGING)
        st = e.read_state()
        for g, L, mask in zip(left["group"].tolist(), left["leader"].tolist(), left["lag_mask"].tolist()):
            for r in range(e.R):
                if mask >> r & 1:                                       # what an install leaves alone: a higher term
                    assert fld(st, e.R, r, "term")[g] > fld(st, e.R, L, "term")[g], (g, r)
    h.close()
