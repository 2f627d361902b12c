"""Leader no-op entries on the GPU (marker `gpu`): raft_engine_append_noops*
and raft_engine_sm_set_noop against the oracle driven through
tests/noop_model.py.  Every comparison is exact."""
import ctypes as C
import importlib

import numpy as np
import pytest

import client_model as CM
import noop_model as NM
import sm_model as M
from helpers import abi, assert_same_logs, high_g0

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


@pytest.mark.parametrize("R,G,variant", NM.PARITY_CASES, ids=[f"R{c[0]}-G{c[1]}-{c[2]}" for c in NM.PARITY_CASES])
def test_parity_with_the_oracle(R, G, variant):
    """40 steps, append_noops over [3, G - 2) with tickets, 3 steps, resolve,
    append_noops again, 20 steps: info, tickets, ticket_cmds, return codes,
    resolve records, state, logs, digest and counter rows equal the oracle's
    under the model, bit for bit."""
    want, _ = NM.host_parity_run(R, G, variant)
    with RaftEngine(abi.make_params(**NM.TM.RM.parity_kw(R, G, variant))) as e:
        got = NM.parity_run(e, f"R{R} G{G} {variant}")
    NM.assert_same_points(got, want, R)


@pytest.mark.parametrize("where,variant", [("bit31", "ring"), ("top", "ring"), ("top", "flat")])
def test_parity_at_the_top_of_the_global_ids(where, variant):
    """A shard that straddles global id 2^31, and one whose last group is
    2^32 - 1: the call indexes by the engine-local group (the ring's rows
    too), the steps after it draw their timer words by the global id."""
    g0 = high_g0(203)[where]
    want, _ = NM.host_parity_run(5, 203, variant, g0)
    with RaftEngine(abi.make_params(g0=g0, **NM.TM.RM.parity_kw(5, 203, variant))) as e:
        got = NM.parity_run(e, f"R5 G203 {variant} {where}")
    NM.assert_same_points(got, want, 5)


def test_host_and_device_forms_agree_with_and_without_tickets():
    """Three engines in one state: the host form with tickets, the host form
    without, the _dev form.  The same info, the same tickets, the same digest;
    the _dev form writes nothing beyond its records."""
    import torch
    R, G = 5, 203
    kw = NM.TM.RM.parity_kw(R, G, "flat")
    g0, n = 3, G - 5
    with RaftEngine(abi.make_params(**kw)) as a, RaftEngine(abi.make_params(**kw)) as b, \
            RaftEngine(abi.make_params(**kw)) as d:
        for e in (a, b, d):
            e.step(40, counters=False)
        info, tk, tc = a.append_noops(g0, n, NM.NOOP, tickets=True)
        assert b.append_noops(g0, n, NM.NOOP) == info and info["appended"] > 0 and info["current"] > 0
        dk = torch.full(((n + 1) * 4,), -7, dtype=torch.int32, device="cuda:0")
        dc = torch.full((n + 1,), -7, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        assert d.append_noops_dev(dk.data_ptr(), dc.data_ptr(), g0, n, NM.NOOP) == info
        raw, rawc = dk.cpu().numpy(), dc.cpu().numpy()
        same(raw[:-4].view(abi.TICKET_DTYPE), tk, "device tickets")
        same(rawc[:-1].view(np.uint32), tc, "device ticket_cmds")
        assert (raw[-4:] == -7).all() and rawc[-1] == -7
        assert a.digest() == b.digest() == d.digest()
        # no arrays at all on the device form, and a second call everywhere: nothing is appended, but where
        # reference mode's ghost tail still shows a stale slot as the leader's last entry
        again = d.append_noops_dev(0, 0, g0, n, NM.NOOP)
        assert again == a.append_noops(g0, n, NM.NOOP) and again["appended"] <= info["ghosted"]
        assert a.digest() == d.digest()
        with pytest.raises(ValueError, match="16-byte"):
            d.append_noops_dev(dk.data_ptr() + 4, dc.data_ptr(), g0, n, NM.NOOP)


@pytest.mark.parametrize("textbook", [False, True], ids=["reference", "textbook"])
def test_crafted_records_on_the_device(textbook):
    """The crafted groups of noop_model.crafted() and crafted_ring() written
    into an engine (the tail cache is rebuilt first): tickets, ticket_cmds and
    info are the ones written out by hand, the state and logs afterwards the
    oracle's under the model, and a second call changes nothing."""
    mode = dict(mode=abi.MODE_TEXTBOOK) if textbook else {}
    for ring in (False, True):
        w, t, c = NM.crafted_ring(textbook) if ring else NM.crafted()
        G, cap = len(w), t.shape[2]
        kw = dict(R=NM.CR, G=G, log_cap=cap, **mode, **(dict(log_window=NM.RING_W) if ring else {}))
        if ring:
            want_tk, want_c, want_info, want_rc = NM.crafted_ring_want(textbook)
        else:
            want_tk, want_c, want_info = NM.crafted_want(textbook)
            want_rc = abi.RAFT_OK
        h = NM.Host(**kw)
        h.o.write_state(w)
        h.o.write_log(t, c)
        assert h.append_noops(0, G, NM.NOOP, tickets=True)[0] == want_info
        with RaftEngine(abi.make_params(**kw)) as e:
            e.write_state(w)
            e.write_log(t, c)
            info, tk, tc = e.append_noops(0, G, NM.NOOP, tickets=True)
            assert info == want_info and e.last_status == want_rc, (ring, info, e.last_status)
            same(tk, want_tk, f"crafted tickets (ring {ring})")
            same(tc, want_c, f"crafted ticket_cmds (ring {ring})")
            st = e.read_state()
            assert np.array_equal(st, h.read_state())
            if not ring:                                            # (a ring keeps the newest slots only)
                assert_same_logs(st, e.read_log(), h.read_log(), NM.CR, "crafted logs")
            dg = e.digest()
            again = e.append_noops(0, G, NM.NOOP + 1)
            assert again["appended"] == 0 and e.digest() == dg
        h.close()


def test_idle_groups_serve_linearizable_reads():
    """The liveness the feature is for.  Textbook mode, no commands, no faults:
    every read begins TERM_UNCOMMITTED; one no-op per group and the steps the
    oracle run needed, and every ticket is COMMITTED and every read ISSUED; with
    the machine's skip on, every key serves 0 and the machines agree."""
    want = NM.host_idle_reads()
    G = NM.LIVE_KW["G"]
    groups = np.arange(G, dtype=np.int64)
    with RaftEngine(abi.make_params(**NM.LIVE_KW)) as e:
        e.sm_configure(NM.LIVE_SLOTS)
        got = NM.idle_reads(e, settle=want["settle"])
        assert (got["before"]["status"] == abi.READ_TERM_UNCOMMITTED).all()
        assert got["info"]["appended"] == G
        assert (got["resolved"]["status"] == CM.COMMITTED).all()
        assert (got["after"]["status"] == abi.READ_ISSUED).all()
        for k in ("warm", "info", "digest"):
            assert got[k] == want[k], (k, got[k], want[k])
        for k in ("before", "tickets", "cmds", "resolved", "after"):
            same(got[k], want[k], k)
        e.sm_set_noop(NM.NOOP)
        assert e.sm_apply()["applied"] > 0
        keys = (np.arange(G, dtype=np.uint64) * 2654435761 % 2 ** 32).astype(np.uint32)
        rec = e.serve_reads(groups, got["after"], keys)
        assert (rec["status"] == abi.READ_SERVED).all() and (rec["value"] == 0).all()
        assert e.sm_check() == 0
        heads, regs = e.sm_read()
        assert (regs == 0).all() and (heads["applied"] >= 0).all() and (heads["applied"].max(axis=1) == 1).all()


def test_stalled_tickets_are_released():
    """An evacuate of replica 0 and a proposal to every group between two
    steps: the tickets still PENDING 30 steps into the new terms are the ones
    the oracle run names, none of them is after append_noops and that run's
    step count, and no group ever had two leaders of a term or a Log Matching
    violation."""
    want = NM.host_stalled_tickets()
    with RaftEngine(abi.make_params(**NM.LIVE_KW)) as e:
        got = NM.stalled_tickets(e, settle=want["settle"])
    assert got["stalled"] == want["stalled"] and len(got["stalled"]) > 0
    assert (got["final"]["status"][got["stalled"]] != CM.PENDING).all()
    assert got["dual"] == 0 and got["matching"] == 0
    for k in ("warm", "moved", "led0", "evacuate", "info", "digest"):
        assert got[k] == want[k], (k, got[k], want[k])
    for k in ("tickets", "later", "noop_tickets", "final"):
        same(got[k], want[k], k)


def test_error_paths():
    """Null info, one array of the pair, groups outside the engine: refused
    with nothing written; n == 0 is RAFT_OK with a zeroed info."""
    R, G = 5, 70
    with RaftEngine(abi.make_params(R=R, G=G, seed=11, log_cap=64, cmd_ppm=100_000)) as e:
        e.step(40, counters=False)
        before = e.digest()
        lib, h = e._lib, e._h
        buf = np.zeros(G * 4, np.int64)
        p = C.c_void_p(buf.ctypes.data)
        info = abi.raft_noop_info()
        for fn in (lib.raft_engine_append_noops, lib.raft_engine_append_noops_dev):
            info.appended = info.current = 5
            assert fn(h, 0, G, 7, None, None, None) == abi.RAFT_EINVAL and b"null info" in lib.raft_last_error()
            assert fn(h, 0, G, 7, p, None, C.byref(info)) == abi.RAFT_EINVAL and info.appended == 0
            assert fn(h, 0, G, 7, None, p, C.byref(info)) == abi.RAFT_EINVAL
            assert b"both or neither" in lib.raft_last_error()
            for g0, n in ((G, 1), (-1, 2), (G - 1, 2), (0, -1)):
                info.current = 5
                assert fn(h, g0, n, 7, None, None, C.byref(info)) == abi.RAFT_ERANGE and info.current == 0
            info.current = 5
            assert fn(h, G, 0, 7, None, None, C.byref(info)) == abi.RAFT_OK and info.current == 0
            assert fn(h, 3, 0, 7, p, p, C.byref(info)) == abi.RAFT_OK
        assert e.digest() == before
        with pytest.raises(RaftError, match="outside the engine"):
            e.append_noops(G - 1, 2)
        for bad in (dict(cmd=-1), dict(cmd=2 ** 32), dict(g0=1.5), dict(n=True)):
            with pytest.raises(ValueError):
                e.append_noops(**bad)
        with pytest.raises(ValueError):
            e.sm_set_noop(2 ** 32)
        assert e.append_noops(5, 0) == dict.fromkeys(abi.NOOP_INFO_FIELDS, 0)
        info_, tk, tc = e.append_noops(5, 0, tickets=True)
        assert len(tk) == len(tc) == 0 and tk.dtype == abi.TICKET_DTYPE
        assert e.digest() == before
        # the host buffers are written to their ends and not beyond
        t2 = np.full((G + 1) * 4, -7, np.int32)
        c2 = np.full(G + 1, 0xFFFFFFF9, np.uint32)
        assert lib.raft_engine_append_noops(h, 0, G, 7, C.c_void_p(t2.ctypes.data), C.c_void_p(c2.ctypes.data),
                                            C.byref(info)) == abi.RAFT_OK
        assert (t2[-4:] == -7).all() and c2[-1] == 0xFFFFFFF9 and (t2[:-4].reshape(-1, 4)[:, 3] != -7).all()
        assert info.appended + info.current + info.no_leader + info.log_full == G


def test_the_machine_passes_over_the_entry_only_when_told():
    """A run whose logs hold no-ops among the harness's commands.  Disabled (the
    default): sm_apply equals sm_model without the skip.  Enabled, on a second
    engine in the same state: sm_model with it -- the same heads, other
    registers.  reset, sm_configure and sm_write leave the setting alone, and
    it may be set before the machine exists."""
    kw = dict(R=5, G=70, seed=11, log_cap=128, mode=abi.MODE_TEXTBOOK, ae_max_entries=4, cmd_ppm=150_000,
              partition_period=40, partition_len=10)
    R, G, cap, S = 5, 70, 128, NM.LIVE_SLOTS

    def run(e):
        infos = []
        for _ in range(4):
            e.step(25, counters=False)
            infos.append(e.append_noops(cmd=NM.NOOP))
            e.step(5, counters=False)
            infos.append(e.sm_apply())
        return infos

    with RaftEngine(abi.make_params(**kw)) as off, RaftEngine(abi.make_params(**kw)) as on:
        on.sm_set_noop(NM.NOOP)                                     # before the machine is configured
        for e in (off, on):
            e.sm_configure(S)
        on.reset()
        on.sm_configure(S)
        a, b = run(off), run(on)
        assert a == b and sum(i.get("appended", 0) for i in a[::2]) > 0
        st, (t, c) = off.read_state(), off.read_log()
        assert off.digest() == on.digest() and (c == NM.NOOP).any()
        plain, skip = M.Machine(G, R, S), M.Machine(G, R, S)
        M.apply(st, t, c, plain, R, cap)
        NM.sm_apply(st, t, c, skip, R, cap, noop=NM.NOOP)
        for e, m, label in ((off, plain, "disabled"), (on, skip, "enabled")):
            heads, regs = e.sm_read()
            assert np.array_equal(heads, m.heads()), label
            assert np.array_equal(regs, m.reg), label
            assert e.sm_check() == 0
        assert (plain.reg == NM.NOOP).any() and not (skip.reg == NM.NOOP).any()
        # sm_write leaves the setting alone; disabling it restores the plain apply
        heads, regs = on.sm_read()
        on.sm_write(np.zeros_like(heads), np.zeros_like(regs))
        on.sm_apply()
        assert np.array_equal(on.sm_read()[1], skip.reg)
        on.sm_set_noop(None)
        on.sm_write(np.zeros_like(heads), np.zeros_like(regs))
        on.sm_apply()
        assert np.array_equal(on.sm_read()[1], plain.reg)


def test_the_service_asserts_leadership():
    """RaftService on an idle textbook engine: read_linearizable answers
    TERM_UNCOMMITTED and with assert_leadership=True leaves the no-ops behind,
    so that the same read after two steps is SERVED; entries() shows the entry
    under its reserved name, and a service that never asks keeps its ids."""
    kw = dict(NM.LIVE_KW, G=8)
    with RaftEngine(abi.make_params(**kw)) as e:
        e.sm_configure(4)
        svc = service.RaftService(e)
        first = svc.commands.intern("x=1")
        e.step(20, counters=False)
        groups = list(range(8))
        assert svc.read_linearizable(groups, ["x=1"] * 8) == [(None, "TERM_UNCOMMITTED")] * 8
        dg = e.digest()
        assert svc.commands.lookup(svc.NOOP_COMMAND) is None
        e.step(2, counters=False)
        assert svc.read_linearizable(groups, ["x=1"] * 8, assert_leadership=True) == [(None, "TERM_UNCOMMITTED")] * 8
        assert e.digest() != dg and svc.commands.lookup(svc.NOOP_COMMAND) == first + 1
        e.step(2, counters=False)
        # register 0 is the one "x=1" maps to; nothing but no-ops was applied: an empty register reads as id 0
        assert svc.read_linearizable(groups, ["x=1"] * 8) == [(svc.commands.name(0), "SERVED")] * 8
        assert svc.assert_leadership() == dict(appended=0, current=8, no_leader=0, log_full=0, ghosted=0)
        g, tk, tc = svc.last_noops
        assert svc.status(g, tk, [svc.NOOP_COMMAND] * 8) == ["COMMITTED"] * 8
        lead = svc.leader(3)
        assert lead.entries() == [f"{lead.currentTerm}: {svc.NOOP_COMMAND}"]
        assert (e.sm_read()[1] == 0).all()
