"""The safety audit on the GPU (marker `gpu`): raft_audit_* against
tests/audit_model.py over the engine's own exported state and logs.  Every
comparison is exact: the ledger (raft_audit_read), the info of every observe and
the full report."""
import ctypes as C
import importlib

import numpy as np
import pytest

import audit_model as AM
import restart_model as RM
from helpers import abi, fld

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


def same_ledger(got, want, label=""):
    if not np.array_equal(got, want):
        g, w = np.argwhere(got != want)[0]
        raise AssertionError(f"{label}: {int((got != want).any(axis=1).sum())} ledgers differ; first group {g} word {w}: "
                             f"{got[g]} vs {want[g]}")


class Shadow:
    """A RaftEngine with an audit whose every observe is checked, as it
    happens, against the model over the engine's own exported state and logs
    and a ledger carried here: the info, raft_audit_read and the full report."""

    def __init__(self, e, ledger=None):
        self.e, self.a = e, e.audit()
        self.W = int(e.p.log_window)
        self.ledger = AM.fresh(e.G, e.R) if ledger is None else ledger.copy()
        if ledger is not None:
            self.a.write(ledger)
        self.totals = AM.zero_info()

    def observe(self, g0=0, n=None, label=""):
        e = self.e
        want, rc = AM.observe(e.read_state(), *e.read_log(), self.ledger, e.R, e.cap, self.W, e.step_index, g0, n)
        assert rc == abi.RAFT_OK
        got = self.a.observe(g0, n)
        assert got == want, (label, got, want)
        same_ledger(self.a.read(), self.ledger, label)
        winfo, wev, _ = AM.report(self.ledger)
        info, ev = self.a.report()
        assert info == winfo, (label, info, winfo)
        same(ev, wev, f"{label}: report")
        for k in ("unknown",) + abi.AUDIT_KINDS:
            self.totals[k] += got[k]
        return got


def load(e, phase):
    st, t, c = phase
    e.write_state(st)
    e.write_log(t, c)


def test_crafted_groups_on_the_device():
    """audit_model.CRAFTED and RING through write_state / write_log: the flags
    written out by hand after each phase, the ledger and info the model's; a
    second audit resumed from the model's ledger after phase 0 (raft_audit_write)
    ends the same; the host and _dev report forms agree."""
    import torch
    for phases, names, R, cap, W, flags in (
            ((AM.crafted_phase(0), AM.crafted_phase(1)), AM.CRAFTED_NAMES, AM.CR, AM.CCAP, 0,
             (AM.crafted_flags(0), AM.crafted_flags(1))),
            ((AM.ring_phase(0), AM.ring_phase(1)), AM.RING_NAMES, AM.CR, AM.RING_CAP, AM.RING_W, None)):
        with RaftEngine(abi.make_params(R=R, G=len(names), log_cap=cap, log_window=W)) as e:
            s = Shadow(e)
            unknown = []
            for k in (0, 1):
                load(e, phases[k])
                e.step_index = AM.CRAFTED_STEPS[k]
                dg = e.digest()
                unknown.append(s.observe(label=f"phase {k}")["unknown"])
                assert e.digest() == dg
                if flags is not None:
                    assert np.array_equal(s.a.read()[:, AM.FLAGS], flags[k])
                if k == 0:
                    after0 = s.ledger.copy()
            if flags is None:
                assert tuple(unknown) == AM.RING_UNKNOWN and not s.a.read()[:, AM.FLAGS].any()
            # resumed from the ledger after phase 0: phase 1 alone gives the same
            r = Shadow(e, after0)
            r.observe(label="resumed")
            same_ledger(r.a.read(), s.a.read(), "resumed")
            # the _dev form: the same records, nothing beyond them
            info, ev = s.a.report()
            buf = torch.full(((len(names) + 1) * 4,), -7, dtype=torch.int32, device="cuda:0")
            torch.cuda.synchronize()
            assert s.a.report_dev(buf.data_ptr(), len(names)) == info
            raw = buf.cpu().numpy()
            same(raw[:len(ev) * 4].view(abi.AUDIT_EVENT_DTYPE), ev, "device events")
            assert (raw[len(ev) * 4:] == -7).all()


PARITY = [(R, mode, W) for R in (1, 3, 5, 8) for mode in ("reference", "textbook") for W in (0, 16)]


@pytest.mark.parametrize("R,mode,W", PARITY, ids=[f"R{r}-{m}-{'ring' if w else 'flat'}" for r, m, w in PARITY])
def test_parity_after_every_observe(R, mode, W):
    """G = 203 under drops, churn, partitions and commands, with persistent and
    amnesia restart_random between launches: after every observe (whole engine
    and sub-ranges, at uneven intervals) the ledger, the info and the full
    report equal the model's."""
    kw = dict(R=R, G=203, seed=11, log_cap=300, log_window=W, **RM.STRESS_MIX)
    if mode == "textbook":
        kw.update(mode=abi.MODE_TEXTBOOK, ae_max_entries=4)
    with RaftEngine(abi.make_params(**kw)) as e:
        s = Shadow(e)
        s.observe(label="fresh")
        e.step(13, counters=False)
        s.observe(label="13")
        e.step(17, counters=False)
        s.observe(5, 100, label="30, groups [5, 105)")
        e.restart(ppm=150_000, down_steps=4)
        e.step(9, counters=False)
        s.observe(label="39, after a persistent restart")
        e.step(1, counters=False)
        s.observe(label="40")
        e.restart(ppm=150_000, amnesia=True)
        amn = s.observe(3, 198, label="40, after an amnesia restart, groups [3, 201)")
        e.step(20, counters=False)
        s.observe(label="60")
        e.restart(ppm=100_000, amnesia=True, down_steps=6)
        e.step(7, counters=False)
        s.observe(label="67")
        assert (s.ledger[:, AM.ACOUNT] > 0).any() and (s.ledger[:, AM.LTERM] > 0).any()
        assert amn["term_regressed"] > 0                                # replicas of a term > 0 forgot it

def test_observe_and_report_never_write_the_engine():
    """raft_engine_digest, read_state, read_applied and read_watch are equal
    before and after observe + report (host and peek forms)."""
    kw = RM.parity_kw(5, 203, "flat")
    with RaftEngine(abi.make_params(**kw)) as e:
        e.step(40, counters=False)
        e.drain_committed()
        e.poll_leaders()
        a = e.audit()
        snap = lambda: (e.digest(), e.read_state(), e.applied(), e.read_watch())
        before = snap()
        a.observe()
        first = snap()
        assert before[0] == first[0] and all(np.array_equal(x, y) for x, y in zip(before[1:], first[1:]))
        e.restart(ppm=300_000, amnesia=True)
        mid = snap()
        info = a.observe()
        assert info["flagged"] > 0
        a.report()
        a.report(max_events=0)
        after = snap()
        assert mid[0] == after[0] and all(np.array_equal(x, y) for x, y in zip(mid[1:], after[1:]))
        assert before[0] != mid[0]                                      # (the restart did change it)
        a.close()


def test_sub_ranges_and_report_cuts():
    """Observes with g0 > 0 and n no multiple of 32 or 64 touch only their
    groups; report cuts at 0 (a peek: pending equals the total), 1, the middle,
    exactly the total and beyond, on a sub-range, host and _dev forms."""
    import torch
    G = 203
    p0, p1, want = AM.bulk(G)
    with RaftEngine(abi.make_params(R=3, G=G, log_cap=16)) as e:
        s = Shadow(e)
        load(e, p0)
        s.observe(label="phase 0")
        load(e, p1)
        e.step_index = 77
        s.observe(9, 83, label="groups [9, 92)")
        L = s.a.read()
        inside = np.zeros(G, bool)
        inside[9:92] = True
        assert np.array_equal(L[:, AM.FLAGS], np.where(inside, want, 0)) and (L[L[:, AM.FLAGS] != 0, AM.FIRST] == 77).all()
        s.observe(101, 97, label="groups [101, 198)")
        g0, n = 5, 150
        _, whole, _ = AM.report(s.ledger, g0, n)
        total = len(whole)
        assert total > 8
        buf = torch.full(((total + 6) * 4,), -7, dtype=torch.int32, device="cuda:0")
        for m in (0, 1, total // 2, total, total + 5):
            winfo, wev, _ = AM.report(s.ledger, g0, n, m)
            info, ev = s.a.report(g0, n, m)
            assert info == winfo and info["pending"] == total - min(m, total)
            same(ev, wev, f"cut {m}")
            buf.fill_(-7)
            torch.cuda.synchronize()
            assert s.a.report_dev(buf.data_ptr() if m else 0, m, g0, n) == winfo
            raw = buf.cpu().numpy()
            same(raw[:len(wev) * 4].view(abi.AUDIT_EVENT_DTYPE), wev, f"device cut {m}")
            assert (raw[len(wev) * 4:] == -7).all()
        same_ledger(s.a.read(), s.ledger, "a report consumes nothing")


def test_past_one_workgroup_and_a_partial_last_wave():
    """G = 70,001, R = 3: states built in numpy and loaded with the write
    calls, never stepped; every 7th group raises one of the five flags in
    rotation at the second observe.  Ledger, info and report are the model's."""
    G = 70_001
    p0, p1, want = AM.bulk(G)
    with RaftEngine(abi.make_params(R=3, G=G, log_cap=16)) as e:
        s = Shadow(e)
        load(e, p0)
        e.step_index = 3
        first = s.observe(label="phase 0")
        assert first["flagged"] == 0 and (s.ledger[:, AM.ACOUNT] == 2).all()
        load(e, p1)
        e.step_index = 4
        info = s.observe(label="phase 1")
        assert np.array_equal(s.a.read()[:, AM.FLAGS], want)
        assert info["flagged"] == info["newly_flagged"] == -(-G // 7)
        assert sorted(info[k] for k in abi.AUDIT_KINDS) == [2000, 2000, 2000, 2000, 2001]
        # a resumed audit on the same state sees what a third observe sees
        r = Shadow(e, s.ledger)
        assert r.observe(label="resumed") == s.observe(label="third")


def test_resume_and_reset():
    """read from one audit, write into a second audit on a second engine in
    the same state: both observe identically from then on; reset equals a fresh
    handle."""
    kw = RM.parity_kw(5, 203, "flat")
    with RaftEngine(abi.make_params(**kw)) as x, RaftEngine(abi.make_params(**kw)) as y:
        for e in (x, y):
            e.step(40, counters=False)
        a = x.audit()
        a.observe()
        for e in (x, y):
            e.restart(ppm=200_000, amnesia=True)
            e.step(5, counters=False)
        b = y.audit()
        b.write(a.read())
        ia, ib = a.observe(), b.observe()
        assert ia == ib and ia["term_regressed"] > 0
        same_ledger(b.read(), a.read(), "resumed")
        same(b.report()[1], a.report()[1], "resumed report")
        fresh_info = y.audit().observe()
        b.reset()
        same_ledger(b.read(), AM.fresh(y.G, y.R), "reset")
        assert b.report()[0] == dict(delivered=0, pending=0, flagged=0)
        assert b.observe() == fresh_info
        x.reset()                                                       # raft_engine_reset does not reach the audit
        assert a.report()[0]["flagged"] == ia["flagged"]


def test_refusals_and_device_bytes():
    """The refusals of include/raft_engine.h: null handle or info, a negative
    max_events, a null buffer with room, a misaligned _dev buffer (RAFT_EINVAL),
    groups outside the engine (RAFT_ERANGE), n == 0 (RAFT_OK, zeroed info); a
    refused raft_audit_write stores nothing; the ledger counts in
    raft_audit_device_bytes and not in raft_engine_device_bytes."""
    import torch
    R, G, cap = 5, 70, 64
    with RaftEngine(abi.make_params(R=R, G=G, seed=11, log_cap=cap, cmd_ppm=100_000)) as e:
        before = e.device_bytes
        a = e.audit()
        assert a.device_bytes >= G * (32 + 8 * R) and e.device_bytes == before
        e.step(40, counters=False)
        a.observe()
        lib, h = e._lib, a._h
        L = a.read()
        ai, ri = abi.raft_audit_info(), abi.raft_audit_report_info()
        buf = np.zeros(G, abi.AUDIT_EVENT_DTYPE)
        p = C.c_void_p(buf.ctypes.data)
        dev = torch.zeros(G * 4 + 8, dtype=torch.int32, device="cuda:0")
        assert lib.raft_audit_observe(None, 0, G, C.byref(ai)) == abi.RAFT_EINVAL
        assert lib.raft_audit_observe(h, 0, G, None) == abi.RAFT_EINVAL and b"null info" in lib.raft_last_error()
        assert lib.raft_audit_create(None, C.byref(C.c_void_p())) == abi.RAFT_EINVAL
        assert lib.raft_audit_create(e._h, None) == abi.RAFT_EINVAL
        assert lib.raft_audit_destroy(None) == abi.RAFT_OK and lib.raft_audit_reset(None) == abi.RAFT_EINVAL
        for g0, n in ((G, 1), (-1, 2), (G - 1, 2), (0, -1)):
            ai.flagged = ai.unknown = 5
            assert lib.raft_audit_observe(h, g0, n, C.byref(ai)) == abi.RAFT_ERANGE
            assert ai.flagged == 0 and ai.unknown == 0
            assert lib.raft_audit_read(h, g0, n, abi.ptr(L, C.c_int32)) == abi.RAFT_ERANGE
        for g0 in (G, 3):
            ai.flagged = 5
            assert lib.raft_audit_observe(h, g0, 0, C.byref(ai)) == abi.RAFT_OK and ai.flagged == 0
        for fn, ptr in ((lib.raft_audit_report, p), (lib.raft_audit_report_dev, C.c_void_p(dev.data_ptr()))):
            assert fn(None, 0, G, ptr, G, C.byref(ri)) == abi.RAFT_EINVAL
            assert fn(h, 0, G, ptr, G, None) == abi.RAFT_EINVAL
            for g0, n, room, rc in ((G, 1, 4, abi.RAFT_ERANGE), (0, G + 1, 4, abi.RAFT_ERANGE), (0, G, -1, abi.RAFT_EINVAL),
                                    (G, 0, 4, abi.RAFT_OK), (3, 0, 0, abi.RAFT_OK)):
                ri.pending = ri.flagged = 5
                assert fn(h, g0, n, ptr, room, C.byref(ri)) == rc, (g0, n, room)
                assert ri.pending == 0 and ri.flagged == 0
            ri.pending = 5
            assert fn(h, 0, G, None, 4, C.byref(ri)) == abi.RAFT_EINVAL and ri.pending == 0
            assert b"null record buffer" in lib.raft_last_error()
        assert lib.raft_audit_report_dev(h, 0, G, C.c_void_p(dev.data_ptr() + 8), 4, C.byref(ri)) == abi.RAFT_EINVAL
        assert b"16-byte" in lib.raft_last_error()
        with pytest.raises(ValueError, match="16-byte"):
            a.report_dev(dev.data_ptr() + 8, 4)
        assert not buf.view(np.int32).any() and not dev.cpu().numpy().any()
        # refused ledgers: through the library itself, nothing stored
        for word, v in ((AM.FLAGS, 32), (AM.FLAGS, -1), (AM.LREP, R), (AM.LREP, -2), (AM.ACOUNT, -1), (AM.ACOUNT, cap + 1)):
            bad = L.copy()
            bad[:, AM.HEAD] += 1                                        # (would be stored in every group if accepted)
            bad[G - 1, word] = v
            assert not AM.valid_ledger(bad, R, cap)
            assert lib.raft_audit_write(h, 0, G, abi.ptr(bad, C.c_int32)) == abi.RAFT_EINVAL
            same_ledger(a.read(), L, "after a refused write")
        edge = L.copy()
        edge[0, AM.ACOUNT], edge[0, AM.LREP], edge[0, AM.FLAGS] = cap, R - 1, abi.AUDIT_ALL
        edge[0, AM.ATERM], edge[0, AM.ASEEN], edge[0, AM.HEAD + 1], edge[0, AM.FIRST] = -7, 2 ** 31 - 1, 99, -1
        a.write(edge)
        same_ledger(a.read(), edge, "the edges of what a write accepts")
        want = edge.copy()
        winfo, _ = AM.observe(e.read_state(), *e.read_log(), want, R, cap, 0, e.step_index)
        assert a.observe() == winfo                                     # no word but those three is an index
        same_ledger(a.read(), want, "observed from the edge ledger")
        with pytest.raises(RaftError, match="outside the engine"):
            a.observe(G - 1, 2)
        a.close()
        a.close()


def test_the_service_end_to_end():
    """RaftService.check_safety on a clean textbook run returns zero flags; the
    same after RaftNode.restart(amnesia=True) on a node with a nonzero term
    reports that group, and `violations` says since when."""
    R, G = 5, 203
    with RaftEngine(abi.make_params(**RM.parity_kw(R, G, "textbook"))) as e:
        svc = service.RaftService(e)
        assert len(svc.violations()) == 0
        for _ in range(3):
            e.step(20, counters=False)
            info = svc.check_safety()
            assert info["flagged"] == 0 and info["unknown"] == 0, info
        assert len(svc.violations()) == 0
        assert (svc.safety_audit.read()[:, AM.ACOUNT] > 0).sum() > G // 2
        st = e.read_state()
        g = int(np.nonzero(fld(st, R, 2, "term") > 0)[0][5])
        svc.node(g, 2).restart(amnesia=True)
        info = svc.check_safety()
        assert info["newly_flagged"] == info["flagged"] == info["term_regressed"] == 1 and svc.last_safety is info
        ev = svc.violations()
        assert ev.dtype == abi.AUDIT_EVENT_DTYPE and len(ev) == 1
        assert (int(ev["group"][0]), int(ev["first_step"][0])) == (g, 60) and int(ev["flags"][0]) & abi.AUDIT_TERM_REGRESSED
        e.step(20, counters=False)
        assert svc.check_safety()["newly_flagged"] == 0 and len(svc.violations(max_events=0)) == 0
        assert len(svc.violations()) >= 1
