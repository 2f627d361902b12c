"""Replica crash and restart on the GPU (marker `gpu`): raft_engine_restart*
against the numpy model of tests/restart_model.py applied to the oracle through
read_state -> model -> write_state.  Every comparison is exact.  That the
inputs are not vacuous is checked on the oracle alone, in test_restart_cpu.py."""
import ctypes as C
import importlib

import numpy as np
import pytest

import restart_model as RM
import sm_model as M
from helpers import abi, assert_same_logs, assert_same_state, fld, log_matching_flags
from test_gpu_parity import handler_messages

pytestmark = pytest.mark.gpu

eng_mod = importlib.import_module("raft-kotlin_amd.engine")
RaftEngine = eng_mod.RaftEngine
RaftError = eng_mod.RaftError
NF = abi.NUM_FIELDS

CASES = [(R, G, v, fl, dn) for R, G, v in RM.PARITY_CASES for fl, dn in RM.PARITY_FLAGS]


def same_everything(e, h, label):
    """State, logs, digest, both cursors and the machine of an engine and a Host."""
    se = e.read_state()
    assert_same_state(se, h.read_state(), e.R, label)
    assert_same_logs(se, e.read_log(), h.read_log(), e.R, label)
    assert e.digest() == h.digest(), f"{label}: digest"
    assert np.array_equal(e.applied(), h.applied()), f"{label}: lastApplied"
    if h.mach:
        (he, re_), (hh, rh) = e.sm_read(), h.sm_read()
        assert np.array_equal(he, hh) and np.array_equal(re_, rh), f"{label}: machine"


def restarted_set(before, after, R):
    """[n, R] bool: the replicas whose own words or session rows changed."""
    n = before.shape[0]
    ch = np.zeros((n, R), bool)
    d = before != after
    for r in range(R):
        ch[:, r] = d[:, r * NF:(r + 1) * NF].any(axis=1) | d[:, R * NF + r * R:R * NF + (r + 1) * R].any(axis=1) | \
            d[:, R * NF + R * R + r * R:R * NF + R * R + (r + 1) * R].any(axis=1)
    return ch


@pytest.mark.parametrize("R,G,variant,flags,down", CASES, ids=[f"R{c[0]}-G{c[1]}-{c[2]}-f{c[3]}-d{c[4]}" for c in CASES])
def test_parity_with_the_oracle(R, G, variant, flags, down):
    """40 steps, a host-mask restart over [3, G - 2), 40 steps, another, 40
    steps; after every leg a drain and an sm_apply.  info, every counter row,
    state, logs, digest, lastApplied and the machine equal the oracle's with
    the model applied by read -> model -> write.  On the ring the comparison
    runs up to the oracle's first window miss, which the engine must count too
    (restart_model.valid_rows: a restarted replica that wins an election replays
    from index 0, below a wrapped window; the run is invalid from there by the
    engine's contract).  The first restart and everything before it are always
    compared; R = 8 and the R = 1 amnesia rings have no miss and compare whole."""
    want, _, _ = RM.host_parity_run(R, G, variant, flags, down)
    with RaftEngine(abi.make_params(**RM.parity_kw(R, G, variant))) as e:
        e.sm_configure(RM.PARITY_SLOTS)
        got = RM.parity_run(e, flags, down)
    RM.assert_same_points(got, want, R)


@pytest.mark.parametrize("ppm", RM.RANDOM_PPM)
def test_random_form(ppm):
    """The seeded rate on a shard whose global ids carry a high bit: the set
    of restarted replicas (every replica has term > 0 by step 40, so with
    amnesia each restarted one shows in the state diff) equals the model's
    selection; a second engine selects the same set; another step index selects
    another."""
    kw = RM.RANDOM_KW
    R, G = kw["R"], kw["G"]
    h = RM.Host(**kw)
    with RaftEngine(abi.make_params(**kw)) as a, RaftEngine(abi.make_params(**kw)) as b:
        sets = []
        for leg in range(2):
            for x in (a, b, h):
                x.step(40)
            before = a.read_state()
            assert all((fld(before, R, r, "term") > 0).all() for r in range(R))
            sel = RM.select_random(kw["seed"], a.step_index, kw["g0"], G, R, ppm)
            info = a.restart(ppm=ppm, amnesia=True)
            assert info == b.restart(ppm=ppm, amnesia=True) == h.restart(ppm=ppm, amnesia=True)
            after = a.read_state()
            got = restarted_set(before, after, R)
            assert np.array_equal(got, sel) and info["restarted"] == int(sel.sum())
            assert np.array_equal(after, b.read_state())
            same_everything(a, h, f"ppm {ppm} leg {leg}")
            sets.append(got)
        assert a.step_index == 80
        if 0 < ppm < 1_000_000:
            assert 0 < sets[0].sum() < sets[0].size and not np.array_equal(sets[0], sets[1])
        else:
            assert sets[0].all() == sets[1].all() == (ppm > 0) and sets[0].any() == (ppm > 0)
        # a sub-range: keyed by the global id, not by the position in the call
        a.step(40)
        before = a.read_state()
        assert all((fld(before, R, r, "term") > 0).all() for r in range(R))
        a.restart(ppm=500_000, g0=57, n=100, amnesia=True)
        want = np.zeros((G, R), bool)
        want[57:157] = RM.select_random(kw["seed"], 120, kw["g0"] + 57, 100, R, 500_000)
        assert np.array_equal(restarted_set(before, a.read_state(), R), want) and 0 < want.sum() < 500
    h.close()


@pytest.mark.parametrize("flags", [0, RM.REPLAY, RM.AMNESIA])
def test_nothing_else_moves(flags):
    """Outside [g0, g0 + n) the digest is unchanged; inside, the unselected
    replicas' words, rows, lastApplied and machines are unchanged."""
    kw = RM.parity_kw(5, 203, "flat")
    R, G, g0, n = 5, 203, 29, 131
    with RaftEngine(abi.make_params(**kw)) as e:
        e.sm_configure(RM.PARITY_SLOTS)
        e.step(40, counters=False)
        e.drain_committed()
        e.sm_apply()
        mask = RM.parity_mask(R, n + 5, 7)
        sel = RM.select_mask(mask, R)
        st0, ap0, (h0, r0) = e.read_state(), e.applied(), e.sm_read()
        lo0, hi0 = e.digest_range(0, g0), e.digest_range(g0 + n, G - g0 - n)
        logs0 = e.read_log()
        info = e.restart(mask, g0=g0, amnesia=bool(flags & RM.AMNESIA), replay=bool(flags & RM.REPLAY), down_steps=6)
        assert info["restarted"] == int(sel.sum()) > 0 and ap0.any() and h0["applied"].any()
        st1, ap1, (h1, r1) = e.read_state(), e.applied(), e.sm_read()
        assert e.digest_range(0, g0) == lo0 and e.digest_range(g0 + n, G - g0 - n) == hi0
        assert np.array_equal(st1[:g0], st0[:g0]) and np.array_equal(st1[g0 + n:], st0[g0 + n:])
        assert_same_logs(st1, e.read_log(), logs0, R, "no log slot below physLen is written")
        full = np.zeros((G, R), bool)
        full[g0:g0 + n] = sel
        keep = np.ones(st0.shape, bool)                                                 # the words of the unselected
        for r in range(R):
            keep[:, r * NF:(r + 1) * NF] &= ~full[:, r:r + 1]
            keep[:, R * NF + r * R:R * NF + (r + 1) * R] &= ~full[:, r:r + 1]
            keep[:, R * NF + R * R + r * R:R * NF + R * R + (r + 1) * R] &= ~full[:, r:r + 1]
        keep[:, -2] = ~full.any(axis=1)                                                 # the isolation word: down_steps
        assert np.array_equal(st1[keep], st0[keep])
        assert np.array_equal(ap1[~full], ap0[~full]) and np.array_equal(h1[~full], h0[~full])
        assert np.array_equal(r1[~full], r0[~full])
        if flags:
            assert not ap1[full].any() and not h1["applied"][full].any() and not h1["hash"][full].any()
            assert not r1[full].any()
        else:
            assert np.array_equal(ap1, ap0) and np.array_equal(h1, h0) and np.array_equal(r1, r0)


@pytest.mark.parametrize("amnesia", [False, True], ids=["persistent", "amnesia"])
@pytest.mark.parametrize("window", [0, 16], ids=["flat", "ring"])
@pytest.mark.parametrize("path", [abi.BATCH_PATH_BUCKETED, abi.BATCH_PATH_SORTED], ids=["bucketed", "sorted"])
def test_cache_and_owner_mirrors(path, window, amnesia):
    """After a restart the log-tail cache, the session rows and the owner word
    are what the handler batches and the step kernel read: a vote batch, an
    append batch and 20 steps, against the oracle doing the same."""
    R, G, cap = 5, 64, 300
    kw = dict(R=R, G=G, seed=11, log_cap=cap, log_window=window, cmd_ppm=500_000, drop_ppm=50_000)
    h = RM.Host(**kw)
    with RaftEngine(abi.make_params(**kw)) as e:
        e.set_batch_path(path)
        ce, ch = e.step(40), h.step(40)
        assert np.array_equal(ce, ch)
        mask = RM.parity_mask(R, G + 5, 3)
        assert e.restart(mask, amnesia=amnesia) == h.restart(mask, amnesia=amnesia)
        assert h.hits["leader"] > 0 and h.hits["restarted"] > 0
        w = h.read_state()
        rng = np.random.default_rng(5 + window)
        grp, dst, vq, aq, _ = handler_messages(rng, 600, G, R, cap, w, window)
        vo = np.array([h.o.vote(int(g), int(d), *map(int, q)) for g, d, q in zip(grp, dst, vq)], dtype=np.int32)
        ao = np.array([(t, int(s), st) for t, s, st in
                       (h.o.append(int(g), int(d), int(q[0]), int(q[1]), int(q[2]), int(q[3]),
                                   (int(q[5]), int(q[6])) if q[4] else None, int(q[7]))
                        for g, d, q in zip(grp, dst, aq))], dtype=np.int32)
        assert np.array_equal(e.vote_batch(grp, dst, vq), vo)
        assert np.array_equal(e.append_batch(grp, dst, aq), ao)
        same_everything(e, h, "after the batches")
        ce, ch = e.step(20), h.step(20)
        # on the ring the run stays valid for as long as the leaders that survived keep their sessions: until a
        # restarted replica (commitIndex 0) wins an election and replays from index 0 (restart_model.valid_rows)
        assert RM.valid_rows(ch) >= 8 and (window or RM.valid_rows(ch) == 20)
        if RM.assert_same_rows(ce, ch, "20 steps after the batches"):
            same_everything(e, h, "after 20 steps")
    h.close()


def test_kernel_choice():
    """down_steps > 0 writes an isolation word, so the next launch runs a kernel
    built for isolation; down_steps = 0 does not."""
    kw = dict(R=5, G=203, seed=11, log_cap=300, cmd_ppm=500_000, partition_period=40, partition_len=10)
    h = RM.Host(**kw)
    mask = RM.parity_mask(5, 203 + 5, 1)
    with RaftEngine(abi.make_params(**kw)) as e:
        assert np.array_equal(e.step(40), h.step(40)) and not e.kernel_info()["net"] & abi.NET_ISO
        assert e.restart(mask, down_steps=0) == h.restart(mask, down_steps=0)
        assert np.array_equal(e.step(10), h.step(10)) and not e.kernel_info()["net"] & abi.NET_ISO
        assert e.restart(mask, down_steps=6) == h.restart(mask, down_steps=6)
        iso, hit = e.read_state()[:, -2], RM.select_mask(mask, 5).any(axis=1)
        assert np.array_equal(iso != 0, hit) and (iso[hit] >> 8 == 6).all() and 0 < hit.sum() < 203
        ce, ch = e.step(10), h.step(10)
        assert e.kernel_info()["net"] & abi.NET_ISO
        assert np.array_equal(ce, ch) and ch[:, abi.C_INDEX["msg_dropped"]].sum() > 0
        same_everything(e, h, "isolated after the restart")
    h.close()


@pytest.mark.parametrize("kind", ["persistent", "replay", "amnesia"])
def test_safety_observers(kind):
    """Textbook mode, flat log: restarts every 20 steps at 10^5 ppm for 200
    steps, an sm_apply and a drain of replica 0 after each launch, in parity
    with the model throughout.  Persistent restarts keep every safety property
    and replica 0's drained stream is its final log prefix, each index once.
    With replay every machine that has caught up is the fold of its log.  With
    amnesia the observers' reports are only recorded (forgetting votes may
    legitimately break safety); parity with the model is still asserted."""
    kw, S = RM.SAFETY_KW, RM.SAFETY_SLOTS
    R, G, cap = kw["R"], kw["G"], kw["log_cap"]
    flags = dict(amnesia=kind == "amnesia", replay=kind == "replay")
    h = RM.Host(S, **kw)
    dual, streams = 0, [[] for _ in range(G)]
    with RaftEngine(abi.make_params(**kw)) as e:
        e.sm_configure(S)
        for k in range(RM.SAFETY_STEPS // 20):
            ce, ch = e.step(20), h.step(20)
            assert np.array_equal(ce, ch), f"{kind} launch {k}"
            dual += int(ce[:, abi.C_INDEX["dual_leader_groups"]].sum())
            assert e.sm_apply() == h.sm_apply()
            (rec, di), (rech, dih) = e.drain_committed(replica=0), h.drain_committed(replica=0)
            assert np.array_equal(rec, rech) and di == dih
            for g, _, i, t, c in rec.tolist():
                streams[g].append((i, t, c))
            assert e.restart(ppm=RM.SAFETY_PPM, **flags) == h.restart(ppm=RM.SAFETY_PPM, **flags)
            same_everything(e, h, f"{kind} launch {k}")
        st, (t, c) = e.read_state(), e.read_log()
        mismatched, diverged = e.check_log_matching(), e.sm_check()
        heads, regs = e.sm_read()
    h.close()
    assert mismatched == int(log_matching_flags(st, t, c, R).sum()) and diverged == int(M.check(h.mach).sum())
    print(f"{kind}: dual_leader_groups {dual}, log matching {mismatched}, sm_check {diverged}")
    if kind == "amnesia":
        return
    assert dual == 0 and mismatched == 0 and diverged == 0
    if kind == "persistent":
        assert sum(len(s) for s in streams) > 1000
        for g, s in enumerate(streams):
            assert [i for i, _, _ in s] == list(range(len(s))), f"group {g}: not one ascending run"
            assert [(tt, cc) for _, tt, cc in s] == list(zip(t[g, 0, :len(s)].tolist(), c[g, 0, :len(s)].tolist()))
    else:
        hi = np.stack([np.clip(np.minimum(fld(st, R, r, "commit"), fld(st, R, r, "last")), 0, cap) for r in range(R)], -1)
        caught_up = np.argwhere(heads["applied"] == hi)
        assert len(caught_up) > G
        for g, r in caught_up:
            m = M.Machine(1, 1, S)
            for i in range(int(hi[g, r])):
                m.apply_entry(0, 0, i, int(t[g, r, i]), int(c[g, r, i]))
            assert int(heads["hash"][g, r]) == int(m.hash[0, 0]) and np.array_equal(regs[g, r], m.reg[0, 0])


def test_errors_and_the_device_mask():
    import torch
    R, G = 3, 40
    kw = dict(R=R, G=G, seed=4, log_cap=64, cmd_ppm=1_000_000)
    lib = abi.load_library()
    with RaftEngine(abi.make_params(**kw)) as e, RaftEngine(abi.make_params(**kw)) as d:
        e.step(30, counters=False)
        d.step(30, counters=False)
        st = e.read_state()
        info = abi.raft_restart_info(7, 7, 7, 7)
        mask = np.full(G, 0b101, np.uint8)
        p = C.c_void_p(mask.ctypes.data)
        forms = [lambda g0, n, fl, dn, inf: lib.raft_engine_restart(e._h, g0, n, p, fl, dn, inf),
                 lambda g0, n, fl, dn, inf: lib.raft_engine_restart_random(e._h, g0, n, 1_000_000, fl, dn, inf)]
        for call in forms:
            for g0, n in ((0, G + 1), (G, 1), (-1, 2), (1, G), (0, -1)):
                assert call(g0, n, 0, 0, C.byref(info)) == abi.RAFT_ERANGE and b"range" in lib.raft_last_error()
            assert call(0, G, 0, 0, None) == abi.RAFT_EINVAL
            assert call(0, G, 4, 0, C.byref(info)) == abi.RAFT_EINVAL and call(0, G, -1, 0, C.byref(info)) == abi.RAFT_EINVAL
            assert call(0, G, 0, -1, C.byref(info)) == abi.RAFT_EINVAL
            assert call(0, G, 0, 1 << 23, C.byref(info)) == abi.RAFT_EINVAL
            info.restarted = info.reserved = 7
            assert call(5, 0, 3, 9, C.byref(info)) == abi.RAFT_OK and call(G, 0, 0, 0, C.byref(info)) == abi.RAFT_OK
            assert (info.restarted, info.leaders, info.entries_dropped, info.reserved) == (0, 0, 0, 0)
        assert lib.raft_engine_restart(e._h, 0, G, None, 0, 0, C.byref(info)) == abi.RAFT_EINVAL
        assert lib.raft_engine_restart_dev(e._h, 0, G, None, 0, 0, C.byref(info)) == abi.RAFT_EINVAL
        assert lib.raft_engine_restart(e._h, 0, 0, None, 0, 0, C.byref(info)) == abi.RAFT_OK
        with pytest.raises(RaftError, match="range"):
            e.restart(mask, g0=1)
        assert np.array_equal(e.read_state(), st)                           # nothing was applied by any of them
        # the largest down_steps fits the isolation word; a device mask made by torch equals the host form
        m = mask.copy()
        m[::3] = 0
        m[4] = 0xF8                                                         # only bits at or above R: nobody
        tm = torch.from_numpy(m).cuda()
        torch.cuda.synchronize()
        a = e.restart(m[2:], g0=2, amnesia=True, down_steps=(1 << 23) - 1)
        b = d.restart_dev(tm.data_ptr() + 2, g0=2, n=G - 2, amnesia=True, down_steps=(1 << 23) - 1)
        assert a == b and a["restarted"] == 2 * int((m[2:] == 0b101).sum()) > 0 and a["entries_dropped"] > 0
        se = e.read_state()
        assert np.array_equal(se, d.read_state()) and e.digest() == d.digest()
        assert se[2, -2] == ((1 << 23) - 1) << 8 and se[1, -2] == 0 and se[3, -2] == 0
        assert np.array_equal(e.step(5), d.step(5))


def test_service_restart():
    svc_mod = importlib.import_module("raft-kotlin_amd.service")
    R = 3
    with RaftEngine(abi.make_params(R=R, G=4, seed=4, log_cap=64, cmd_ppm=1_000_000)) as e:
        e.step(60, counters=False)
        svc = svc_mod.RaftService(e)
        led = np.flatnonzero(e.leaders()["leader"] >= 0)
        assert len(led) > 0
        lead = svc.leader(int(led[0]))
        assert lead is not None and lead.entries() and lead.currentTerm > 0 and lead.state == "LEADER"
        other = svc.node(lead.group, (lead.replica + 1) % R)
        kept = other.entries(), other.currentTerm
        info = lead.restart(amnesia=True)
        assert info == dict(restarted=1, leaders=1, entries_dropped=info["entries_dropped"]) and info["entries_dropped"] > 0
        assert lead.entries() == [] and lead.currentTerm == 0 and lead.state == "FOLLOWER" and lead.votedFor == -1
        assert (other.entries(), other.currentTerm) == kept
        # several nodes in one call, one of them named twice; a persistent restart keeps term and log
        n0, n1 = svc.node(0, 1), svc.node(3, 2)
        before = n0.entries(), n0.currentTerm, n1.entries(), n1.currentTerm
        assert svc.restart([3, 0, 3], [2, 1, 2])["restarted"] == 2
        assert (n0.entries(), n0.currentTerm, n1.entries(), n1.currentTerm) == before
        assert n0.commitIndex == 0 and n1.commitIndex == 0 and n0.state == "FOLLOWER"
        assert svc.restart([], []) == dict(restarted=0, leaders=0, entries_dropped=0)
        with pytest.raises(IndexError):
            svc.restart([4], [0])
