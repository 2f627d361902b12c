"""Snapshot install on the GPU (marker `gpu`): raft_engine_install_snapshot*
against the numpy model of tests/snapshot_model.py applied to the oracle through
read_state / read_log -> model -> write_state / write_log.  Every comparison is
exact.  That the inputs are not vacuous is checked on the oracle alone, in
test_snapshot_cpu.py."""
import ctypes as C
import importlib

import numpy as np
import pytest

import restart_model as RM
import snapshot_model as SM
from helpers import abi, assert_same_logs, assert_same_state, fld
from test_gpu_parity import handler_messages

pytestmark = pytest.mark.gpu

eng_mod = importlib.import_module("raft-kotlin_amd.engine")
svc_mod = importlib.import_module("raft-kotlin_amd.service")
RaftEngine = eng_mod.RaftEngine
RaftError = eng_mod.RaftError
NF = abi.NUM_FIELDS
ZERO_INFO = dict.fromkeys(SM.INFO_KEYS, 0)


def same_engines(a, b, label):
    """State, logs, digest and the machine of two engines (or an engine and a Host)."""
    sa = a.read_state()
    assert_same_state(sa, b.read_state(), a.R, label)
    assert_same_logs(sa, a.read_log(), b.read_log(), a.R, label)
    assert a.digest() == b.digest(), f"{label}: digest"
    (ha, ra), (hb, rb) = a.sm_read(), b.sm_read()
    assert np.array_equal(ha, hb) and np.array_equal(ra, rb), f"{label}: machine"


@pytest.mark.parametrize("R,G,variant", RM.PARITY_CASES, ids=[f"R{c[0]}-G{c[1]}-{c[2]}" for c in RM.PARITY_CASES])
def test_parity_with_the_oracle(R, G, variant):
    """snapshot_model.parity_run on the engine against the cached host run:
    infos, every counter row, state, logs, digest, lastApplied, heads and
    registers bit for bit (restart_model.assert_same_points), on a ring up to
    the oracle's first window miss, which the engine must count too."""
    want, _, _ = SM.host_parity_run(R, G, variant)
    with RaftEngine(abi.make_params(**RM.parity_kw(R, G, variant))) as e:
        e.sm_configure(RM.PARITY_SLOTS)
        got = SM.parity_run(e)
    RM.assert_same_points(got, want, R)


def test_nothing_else_moves():
    """After an install with a sparse mask over [g0, g0 + n): every word of
    every replica that was not installed, every group outside the range and
    every lastApplied is unchanged; in an installed replica's group only the
    leader's next[L][f] / match[L][f] differ besides the replica's own words.
    What did change is the model's result."""
    kw = RM.parity_kw(5, 203, "flat")
    R, G, g0, n = 5, 203, 29, 131
    with RaftEngine(abi.make_params(**kw)) as e:
        e.sm_configure(RM.PARITY_SLOTS)
        e.step(88, counters=False)
        e.drain_committed()
        e.sm_apply()
        mask = SM.install_mask(R, n + 5, 7)
        mask[np.random.default_rng(3).random(n) < 0.6] = 0
        st0, ap0, (h0, r0), (t0, c0) = e.read_state(), e.applied(), e.sm_read(), e.read_log()
        lo0, hi0 = e.digest_range(0, g0), e.digest_range(g0 + n, G - g0 - n)
        info = e.install_snapshot(mask, g0=g0)
        st1, ap1, (h1, r1), (t1, c1) = e.read_state(), e.applied(), e.sm_read(), e.read_log()
        assert e.digest_range(0, g0) == lo0 and e.digest_range(g0 + n, G - g0 - n) == hi0
        emin, emax = int(e.p.election_min_ms), int(e.p.election_max_ms)
    # the model on the words read before
    want, wt, wc, wh, wr = st0.copy(), t0.copy(), c0.copy(), h0.copy(), r0.copy()
    done = []
    winfo = SM.install(want[g0:g0 + n], wt[g0:g0 + n], wc[g0:g0 + n], wh[g0:g0 + n], wr[g0:g0 + n], RM.select_mask(mask, R),
                       R=R, cap=kw["log_cap"], W=0, seed=kw["seed"], step=88, gid0=g0, emin=emin, emax=emax, installed=done)
    assert info == winfo and 0 < info["installed"] < n and info["slots_copied"] > 0
    assert_same_state(st1, want, R, "the installed words")
    assert_same_logs(st1, (t1, c1), (wt, wc), R, "the installed logs")
    assert np.array_equal(h1, wh) and np.array_equal(r1, wr)
    # and nothing else
    keep = np.ones(st0.shape, bool)
    inst = np.zeros((G, R), bool)
    for j, L, f in done:
        g = g0 + j
        inst[g, f] = True
        keep[g, f * NF:(f + 1) * NF] = False
        keep[g, R * NF + f * R:R * NF + (f + 1) * R] = False
        keep[g, R * NF + R * R + f * R:R * NF + R * R + (f + 1) * R] = False
        keep[g, R * NF + L * R + f] = keep[g, R * NF + R * R + L * R + f] = False
    assert np.array_equal(st1[keep], st0[keep])
    assert np.array_equal(st1[:g0], st0[:g0]) and np.array_equal(st1[g0 + n:], st0[g0 + n:])
    assert np.array_equal(ap1, ap0) and ap0.any()
    assert np.array_equal(h1[~inst], h0[~inst]) and np.array_equal(r1[~inst], r0[~inst])
    assert np.array_equal(t1[~inst], t0[~inst]) and np.array_equal(c1[~inst], c0[~inst])


def test_installed_ex_leader():
    """A deposed leader with a shorter log (snapshot_model.craft_ex_leader) is
    installed as the model says, and the run goes on in parity with the oracle."""
    h = SM.Host(RM.PARITY_SLOTS, **SM.EX_LEADER_KW)
    with RaftEngine(abi.make_params(**SM.EX_LEADER_KW)) as e:
        e.sm_configure(RM.PARITY_SLOTS)
        g, L, f = SM.craft_ex_leader(e)
        assert (g, L, f) == SM.craft_ex_leader(h)
        st = e.read_state()
        assert fld(st, e.R, f, "role")[g] == abi.LEADER and fld(st, e.R, f, "term")[g] < fld(st, e.R, L, "term")[g]
        m = np.array([1 << f], np.uint8)
        assert e.install_snapshot(m, g0=g) == h.install_snapshot(m, g0=g)
        assert h.ihits["ex_leader"] == 1
        same_engines(e, h, "after the install")
        assert np.array_equal(e.step(20), h.step(20))
        same_engines(e, h, "20 steps later")
    h.close()


@pytest.mark.parametrize("window", [0, 16], ids=["flat", "ring"])
@pytest.mark.parametrize("path", [abi.BATCH_PATH_BUCKETED, abi.BATCH_PATH_SORTED], ids=["bucketed", "sorted"])
def test_cache_and_owner_mirrors(path, window):
    """After an install the log-tail cache, the session rows and the owner word
    are what the step kernel and the handler batches read: the install, 20
    steps and a vote and an append batch on one engine equal the host route
    (write_state + write_log + sm_write of the same words, which rebuilds the
    cache and moves every session row to spill) followed by the same on another."""
    R, G, cap = 5, 64, 300
    kw = dict(R=R, G=G, seed=11, log_cap=cap, log_window=window, cmd_ppm=500_000, drop_ppm=50_000, churn_ppm=20_000,
              churn_steps=15)
    with RaftEngine(abi.make_params(**kw)) as e, RaftEngine(abi.make_params(**kw)) as d:
        for x in (e, d):
            x.set_batch_path(path)
            x.sm_configure(RM.PARITY_SLOTS)
            for _ in range(6):                                         # applied often enough that no ring leader is gapped
                x.step(10, counters=False)
                x.sm_apply()
        mask = SM.install_mask(R, G + 5, 3)
        info = e.install_snapshot(mask)
        assert info == SM.install_engine_like(d, RM.select_mask(mask, R), g0=0) and info["installed"] > 20
        same_engines(e, d, "after the install")
        if not RM.assert_same_rows(e.step(20), d.step(20), "20 steps later"):
            return                                                     # a window miss: invalid from there (not expected)
        same_engines(e, d, "20 steps later")
        w = e.read_state()
        grp, dst, vq, aq, _ = handler_messages(np.random.default_rng(5 + window), 600, G, R, cap, w, window)
        assert np.array_equal(e.vote_batch(grp, dst, vq), d.vote_batch(grp, dst, vq))
        assert np.array_equal(e.append_batch(grp, dst, aq), d.append_batch(grp, dst, aq))
        same_engines(e, d, "after the batches")
        if RM.assert_same_rows(e.step(5), d.step(5), "5 steps after the batches"):
            assert e.digest() == d.digest()


@pytest.mark.parametrize("healed", [False, True], ids=["A-no-install", "B-healed"])
def test_ring_stays_valid(healed):
    """The validity scenario on the engine.  Run B (healed by RaftService.heal)
    equals the oracle's bit for bit and counts no window miss, no dual leader,
    no log mismatch, no diverged machine and no lost entry.  Run A (no install)
    equals the oracle's rows up to its first window miss and counts one there."""
    want, _, _ = SM.host_validity_run(healed)
    with RaftEngine(abi.make_params(**SM.VALID_KW)) as e:
        e.sm_configure(SM.VALID_SLOTS)
        svc = svc_mod.RaftService(e)
        got = SM.validity_run(e, (lambda x: svc.heal()) if healed else None)
        mismatched, diverged = e.check_log_matching(), e.sm_check()
    c = got["counters"]
    if not healed:
        assert not RM.assert_same_rows(c, want["counters"], "run A") and c[:, abi.C_INDEX["log_window_miss"]].sum() > 0
        return
    SM.assert_same_run(got, want, SM.VALID_KW["R"], "run B")
    assert sum(i.get("installed", 0) for i in got["infos"]) > 100
    assert c[:, abi.C_INDEX["log_window_miss"]].sum() == 0 and c[:, abi.C_INDEX["dual_leader_groups"]].sum() == 0
    assert mismatched == 0 and diverged == 0 and not got["heads"]["lost"].any()


def test_reads_after_install():
    """Both followers of every group with a leader lose their machines (a REPLAY
    restart), are installed from the leader, and where one of them becomes the
    leader it serves a SERVED linearizable read of a key written before the
    install, from registers it never folded itself.  (With lockstep timers some
    groups of three never elect anybody: the reference's livelock.  The groups
    that do are the ones read.)"""
    R, G = 3, 16
    kw = dict(R=R, G=G, seed=4, log_cap=128, mode=abi.MODE_TEXTBOOK, ae_max_entries=4)
    with RaftEngine(abi.make_params(**kw)) as e:
        e.sm_configure(8)
        svc = svc_mod.RaftService(e)
        e.step(40, counters=False)
        old = e.leaders()["leader"].copy()
        led = np.flatnonzero(old >= 0)
        assert len(led) >= 4
        tk = svc.submit(led, ["k1"] * len(led))
        e.step(6, counters=False)
        assert svc.status(led, tk, ["k1"] * len(led)) == ["COMMITTED"] * len(led)
        svc.apply_committed()
        followers = np.where(old >= 0, 0b111 & ~(1 << np.maximum(old, 0)), 0).astype(np.uint8)
        assert e.restart(followers, replay=True)["restarted"] == 2 * len(led)
        assert not e.sm_read()[0]["applied"][RM.select_mask(followers, R)].any()
        info = e.install_snapshot(followers)
        assert info == {**ZERO_INFO, "installed": 2 * len(led), "slots_copied": info["slots_copied"], "no_leader": G - len(led)}
        heads, regs = e.sm_read()
        for g in led:
            assert (heads[g] == heads[g, old[g]]).all() and (regs[g] == regs[g, old[g]]).all() and heads[g, 0]["applied"] > 0
        # the old leaders leave: cut off for longer than an election takes
        gone = np.where(old >= 0, 1 << np.maximum(old, 0), 0).astype(np.uint8)
        assert e.restart(gone, down_steps=80)["leaders"] == len(led)
        e.step(30, counters=False)
        new = e.leaders()["leader"]
        ok = led[(new[led] >= 0) & (new[led] != old[led])]
        assert len(ok) >= 2, (old, new)
        tk = svc.submit(ok, ["k2"] * len(ok))                          # an entry of the new term must commit first
        e.step(6, counters=False)
        assert svc.status(ok, tk, ["k2"] * len(ok)) == ["COMMITTED"] * len(ok)
        assert svc.read_linearizable(ok, ["k1"] * len(ok)) == [("k1", "SERVED")] * len(ok)
        assert (svc.last_read[0]["replica"] == new[ok]).all()


def test_errors_and_the_device_mask():
    import torch
    R, G = 3, 40
    kw = dict(R=R, G=G, seed=4, log_cap=64, cmd_ppm=1_000_000, drop_ppm=100_000)
    lib = abi.load_library()
    with RaftEngine(abi.make_params(**kw)) as e, RaftEngine(abi.make_params(**kw)) as d:
        for x in (e, d):
            x.step(30, counters=False)
        st = e.read_state()
        info = abi.raft_install_info()
        mask = np.full(G, 0b111, np.uint8)
        p = C.c_void_p(mask.ctypes.data)
        # not configured: RAFT_EINVAL like every raft_engine_sm_* call, in both forms
        for fn in (lib.raft_engine_install_snapshot, lib.raft_engine_install_snapshot_dev):
            assert fn(e._h, 0, G, p, 0, C.byref(info)) == abi.RAFT_EINVAL and b"configure" in lib.raft_last_error()
            assert fn(None, 0, G, p, 0, C.byref(info)) == abi.RAFT_EINVAL
        with pytest.raises(RaftError, match="configure"):
            e.install_snapshot()
        for x in (e, d):
            x.sm_configure(4)
            x.sm_apply()
        for fn in (lib.raft_engine_install_snapshot, lib.raft_engine_install_snapshot_dev):
            assert fn(e._h, 0, G, p, 0, None) == abi.RAFT_EINVAL
            assert fn(e._h, 0, G, p, -1, C.byref(info)) == abi.RAFT_EINVAL and b"min_lag" in lib.raft_last_error()
            for g0, n in ((0, G + 1), (G, 1), (-1, 2), (1, G), (0, -1)):
                assert fn(e._h, g0, n, p, 0, C.byref(info)) == abi.RAFT_ERANGE and b"range" in lib.raft_last_error()
            info.installed = info.slots_copied = info.no_leader = info.leader_gapped = info.ahead = 7
            info.reserved[0] = info.reserved[2] = 7
            assert fn(e._h, 5, 0, p, 0, C.byref(info)) == abi.RAFT_OK and fn(e._h, G, 0, None, 3, C.byref(info)) == abi.RAFT_OK
            assert [getattr(info, k) for k in SM.INFO_KEYS] + list(info.reserved) == [0] * 8
        with pytest.raises(ValueError, match="min_lag"):
            e.install_snapshot(min_lag=-1)
        with pytest.raises(RaftError, match="range"):
            e.install_snapshot(mask, g0=1)
        assert np.array_equal(e.read_state(), st)                           # nothing was applied by any of them
        # a device mask made by torch equals the host form; bits at or above R name nobody
        m = mask.copy()
        m[::3] = 0
        m[4] = 0xF8
        tm = torch.from_numpy(m).cuda()
        torch.cuda.synchronize()
        a = e.install_snapshot(m[2:], g0=2)
        b = d.install_snapshot(device_mask=tm.data_ptr() + 2, g0=2, n=G - 2)
        assert a == b and a["installed"] > 0
        same_engines(e, d, "device mask == host mask")
        left_out = [0, 1, 3, 4, 6, 9]                                       # before g0, a zero byte, only high bits
        assert np.array_equal(e.read_state()[left_out], st[left_out])
        # a NULL mask is every replica: the 0xFF mask
        a = e.install_snapshot(min_lag=1)
        assert a == d.install_snapshot(np.full(G, 0xFF, np.uint8), min_lag=1)
        same_engines(e, d, "NULL mask == 0xFF mask")
        assert np.array_equal(e.step(5), d.step(5))


def test_service_heal():
    """RaftService.heal (an apply, then an install of every group with the
    default min_lag) and RaftNode.install (this node only)."""
    R, G, W = 3, 6, 16
    kw = dict(R=R, G=G, seed=4, log_cap=128, log_window=W, mode=abi.MODE_TEXTBOOK, ae_max_entries=4, cmd_ppm=1_000_000)
    with RaftEngine(abi.make_params(**kw)) as e:
        e.sm_configure(8)
        svc = svc_mod.RaftService(e)
        for _ in range(12):
            e.step(5, counters=False)
            info = svc.heal()
            assert info["leader_gapped"] == 0 and info["ahead"] == 0, info
        assert svc.last_heal_apply["lost"] == 0
        g = int(np.flatnonzero(e.leaders()["leader"] >= 0)[0])          # lockstep timers: some groups of three elect nobody
        lead = svc.leader(g)
        other = svc.node(g, (lead.replica + 1) % R)
        third = svc.node(g, (lead.replica + 2) % R)
        assert len(lead.log()) > W
        other.restart(amnesia=True)
        assert other.log() == [] and other.machine()[0]["applied"] == 0
        info = svc.heal()
        assert info == {**ZERO_INFO, "installed": 1, "slots_copied": W, "no_leader": info["no_leader"]}
        assert other.log() == lead.log() and other.currentTerm == lead.currentTerm and other.commitIndex == lead.commitIndex
        assert other.state == "FOLLOWER" and other.machine()[0] == lead.machine()[0]
        assert np.array_equal(other.machine()[1], lead.machine()[1])
        # one node: the others are not eligible; the leader itself and a node level with it under min_lag do nothing
        third.restart(replay=True)
        assert third.machine()[0]["applied"] == 0
        assert lead.install() == ZERO_INFO and third.install(min_lag=100) == ZERO_INFO
        assert third.install() == {**ZERO_INFO, "installed": 1, "slots_copied": W}
        assert third.machine()[0] == lead.machine()[0] and np.array_equal(third.machine()[1], lead.machine()[1])
        # a flat log's default: a quarter of log_cap
    with RaftEngine(abi.make_params(R=R, G=G, seed=4, log_cap=64, cmd_ppm=1_000_000)) as e:
        e.sm_configure(8)
        svc = svc_mod.RaftService(e)
        e.step(50, counters=False)
        lead = svc.leader(int(np.flatnonzero(e.leaders()["leader"] >= 0)[0]))
        n = len(lead.log())
        assert n > 16
        svc.node(lead.group, (lead.replica + 1) % R).restart(amnesia=True)
        assert svc.heal(min_lag=n + 100)["installed"] == 0 and svc.heal()["installed"] >= 1
