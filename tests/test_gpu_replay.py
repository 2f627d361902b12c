"""WAL replay on the GPU (marker `gpu`): raft_wal_replay* against the source
engine, the host recover, and the numpy model of tests/replay_model.py.  Every
comparison is exact.

The shapes: 67 groups (the last wave of the side paths is partial at every R),
log_cap 512, one command a step, so that a replica gains more than 256 entries
before a late first poll and one run of a batch spans waves and a workgroup
boundary; R = 3, 5, 8 on a flat log and R = 5 with log_window 16, run until the
rings have wrapped many times.

Two facts about the inputs, asserted where they are used.  (1) The election
timeout is drawn at the step index of the replay that touches a replica, so
before a twin is compared with the restarted source every replica of it is
touched once more at that step, by a HARDSTATE of its own term and vote: a
replay like any other.  (2) The source's replicas end with physLen ==
lastIndex: slots a flat log keeps past lastIndex are read by the textbook
append handler, and the stream (rightly) does not carry them.  The group's two
harness words (isolation, commands issued) are not replica state: the twin
never ran the harness, and they are compared apart."""
import ctypes as C
import functools
import importlib
import re

import numpy as np
import pytest

import replay_model as RP
import wal_model as M
from helpers import abi, fld

pytestmark = pytest.mark.gpu

eng_mod = importlib.import_module("raft-kotlin_amd.engine")
svc_mod = importlib.import_module("raft-kotlin_amd.service")
rpl = importlib.import_module("raft-kotlin_amd.replay")
RaftEngine, RaftError = eng_mod.RaftEngine, eng_mod.RaftError

G, CAP, STEPS, EVERY, MORE = 67, 512, 300, 5, 100
NF = abi.NUM_FIELDS


def flat(R):
    return dict(R=R, G=G, seed=11, log_cap=CAP, mode=abi.MODE_TEXTBOOK, ae_max_entries=4, cmd_ppm=1_000_000,
                drop_ppm=50_000, partition_period=150, partition_len=10)


CASES = {"R3": flat(3), "R5": flat(5), "R8": flat(8),
         # the ring: drops and a partition every 150 steps, a command every fourth step, so that a replica cut off
         # for 10 steps is never more than log_window entries behind: nothing is lost and TRUNCATEs occur
         "ring": dict(R=5, G=G, seed=11, log_cap=CAP, mode=abi.MODE_TEXTBOOK, ae_max_entries=4, cmd_ppm=250_000,
                      drop_ppm=50_000, partition_period=150, partition_len=10, log_window=16)}
MODEL_CASE = "R3"


def touch_all(e):
    """Every replica of `e` named once, by a HARDSTATE of its own term and vote."""
    st = e.read_state()
    return M.records([(g, r, M.HS, -1, int(fld(st, e.R, r, "term")[g]), 0, int(fld(st, e.R, r, "voted")[g]))
                      for g in range(e.G) for r in range(e.R)])


def snapshot(e):
    return e.read_state(), e.read_log()


@functools.lru_cache(maxsize=None)
def run(case):
    """Engine A stepped STEPS faulted textbook steps and polled every EVERY
    steps by four streams of its own; every piece replayed into a fresh twin
    whose step index is A's: B7 (the poll's records in pieces of 7), B1000
    (polls of 1000 records), Bdev (poll_dev of 1000 records into a torch buffer,
    replay_dev from it) and Bkeep (whole polls, keep_volatile).  On a flat log a
    fifth stream is polled once, at the end, into Blate as one batch.  Then A
    restarts every replica and everything is stepped MORE steps.  Computed
    once per case; read-only."""
    import torch
    kw = CASES[case]
    R, W = kw["R"], kw.get("log_window", 0)
    out = {"R": R, "W": W, "infos": [], "model_infos": [], "model_bad": []}
    params = lambda: abi.make_params(**kw)                                    # noqa: E731
    with RaftEngine(params()) as A, RaftEngine(params()) as B7, RaftEngine(params()) as B1000, \
            RaftEngine(params()) as Bdev, RaftEngine(params()) as Bkeep, RaftEngine(params()) as Blate:
        w7, w1000, wdev, wlate = A.wal(), A.wal(), A.wal(), A.wal()
        buf = torch.zeros(1000 * 24, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        out["fresh"] = Bkeep.read_state()
        model = case == MODEL_CASE
        if model:
            ms, (mt, mc) = B7.read_state(), tuple(np.zeros_like(a) for a in B7.read_log())
        tot = dict.fromkeys(RP.INFO_KEYS + ("polled", "cut_polls", "dev_cut_polls", "max_piece_run"), 0)
        for _ in range(STEPS // EVERY):
            A.step(EVERY, counters=False)
            for B in (B7, B1000, Bdev, Bkeep):
                B.step_index = A.step_index
            rec, info = w7.poll()
            assert info["lost"] == 0 and info["regressed"] == 0, info     # on the ring: polled often enough
            tot["polled"] += len(rec)
            for piece in RP.pieces(rec, 7):
                got = rpl.replay(B7, piece)
                for k in RP.INFO_KEYS:
                    tot[k] += got[k]
                if model:
                    want = RP.replay_into(B7, piece, ms, mt, mc)
                    if got != want:
                        out["model_infos"].append((got, want))
            if model:
                st, (t, c) = snapshot(B7)
                if not np.array_equal(st, ms):
                    out["model_bad"].append(("state", A.step_index, np.argwhere(st != ms)[:3].tolist()))
                out["model_bad"] += [("log", A.step_index, x) for x in
                                     RP.persistent_errors(st, t, c, ms, mt, mc, R, CAP, W)[:3]]
            rpl.replay(Bkeep, rec, keep_volatile=True)
            while True:
                rec, info = w1000.poll(max_records=1000)
                rpl.replay(B1000, rec)
                tot["cut_polls"] += info["pending"] > 0
                if not info["pending"]:
                    break
            while True:
                info = wdev.poll_dev(buf.data_ptr(), 1000)
                rpl.replay_dev(Bdev, buf.data_ptr(), info["delivered"])
                tot["dev_cut_polls"] += info["pending"] > 0
                if not info["pending"]:
                    break
        twins = {"B7": B7, "B1000": B1000, "Bdev": Bdev}
        if not W:
            Blate.step_index = A.step_index
            rec, info = wlate.poll()
            key = rec["group"].astype(np.int64) * 8 + rec["replica"]
            tot["max_piece_run"] = int(np.unique(key, return_counts=True)[1].max())
            out["late_info"] = rpl.replay(Blate, rec)
            twins["Blate"] = Blate
        out["source_before_restart"] = A.read_state()
        info = A.restart(np.full(G, 0xFF, dtype=np.uint8))
        assert info["restarted"] == G * R
        out["A"] = snapshot(A)
        out["keep"] = snapshot(Bkeep)
        for name, B in twins.items():
            if name != "Blate":                                           # (its one batch named every replica at this step)
                assert rpl.replay(B, touch_all(B))["replicas"] == G * R
            out[name] = snapshot(B)
        out["counters"] = {name: B.step(MORE)[:, : abi.NUM_COUNTERS] for name, B in dict(twins, A=A).items()}
        out["tot"] = tot
    return out


def same_replica_words(a, b, R, label, skip=("phys",)):
    for r in range(R):
        for name in abi.FIELD_NAMES:
            if name not in skip:
                assert np.array_equal(fld(a, R, r, name), fld(b, R, r, name)), \
                    f"{label}: r{r}.{name} differs in groups {np.flatnonzero(fld(a, R, r, name) != fld(b, R, r, name))[:5]}"
    assert np.array_equal(a[:, R * NF:-2], b[:, R * NF:-2]), f"{label}: session rows differ"


def same_logs(sa, la, lb, R, W, label):
    """Equal on [0, lastIndex) -- on a ring, on the part of it both retain."""
    idx = np.arange(CAP)[None, :]
    for r in range(R):
        last = fld(sa, R, r, "last")
        lo = np.maximum(0, np.maximum(fld(sa, R, r, "phys"), last) - W) if W else np.zeros_like(last)
        m = (idx >= lo[:, None]) & (idx < last[:, None])
        assert m.any(), label
        for x, y in zip(la, lb):
            assert np.array_equal(np.where(m, x[:, r], 0), np.where(m, y[:, r], 0)), f"{label}: log of replica {r} differs"


@pytest.mark.parametrize("case", list(CASES))
def test_twin_equals_the_restarted_source(case):
    """1.  A fresh engine that replayed every poll of A equals A after every
    replica restarted with its disk intact: state, logs, and the next 100
    steps' counters (which is what shows the tail cache and the session
    placement are right)."""
    o = run(case)
    R, W, tot = o["R"], o["W"], o["tot"]
    sa, la = o["A"]
    src = o["source_before_restart"]
    assert all(np.array_equal(fld(src, R, r, "phys"), fld(src, R, r, "last")) for r in range(R))     # fact (2)
    assert not src[:, -2].any()                                                                         # no isolation word
    assert tot["malformed"] == 0 and tot["applied"] == tot["polled"] > 10_000, tot
    assert tot["hardstates"] > 0 and tot["entries"] > 0 and tot["truncates"] > 0, tot
    assert tot["cut_polls"] > 0 or case not in ("R5", "R8"), tot          # 335 replicas or more gain 5 entries a poll
    if W:
        assert max(fld(sa, R, r, "last").max() for r in range(R)) > 4 * W                              # wrapped
    else:
        assert tot["max_piece_run"] > 256 + 2, tot                         # one run over a workgroup boundary
        assert o["late_info"]["replicas"] == G * R and o["late_info"]["applied"] > 256 * G
    for name in ("B7", "B1000") + (() if W else ("Blate",)):
        sb, lb = o[name]
        same_replica_words(sa, sb, R, f"{case} {name}")
        assert all(np.array_equal(fld(sb, R, r, "phys"), fld(sb, R, r, "last")) for r in range(R)), name
        assert not sb[:, -2:].any()                                        # the twin never ran the harness
        same_logs(sa, la, lb, R, W, f"{case} {name}")
        assert np.array_equal(o["counters"][name], o["counters"]["A"]), \
            f"{case} {name}: counters differ at step {np.argwhere(o['counters'][name] != o['counters']['A'])[0]}"
    ca = o["counters"]["A"]
    assert ca[:, abi.C_INDEX["leaders_elected"]].sum() > 0 and ca[:, abi.C_INDEX["commits"]].sum() > 0


@pytest.mark.parametrize("case", list(CASES))
def test_device_path_equals_the_host_path(case):
    """2.  poll_dev into a torch buffer and replay_dev from it, no host copy of
    a record: the twin is B1000, word for word."""
    o = run(case)
    assert o["tot"]["dev_cut_polls"] > 0 or case not in ("R5", "R8"), o["tot"]
    (sd, ld), (sb, lb) = o["Bdev"], o["B1000"]
    assert np.array_equal(sd, sb)
    assert np.array_equal(ld[0], lb[0]) and np.array_equal(ld[1], lb[1])
    assert np.array_equal(o["counters"]["Bdev"], o["counters"]["A"])


def test_replays_equal_the_model():
    """4.  Every replay of B7 in the R = 3 run: its info equals the model's, and
    after every poll's pieces the twin's state and logs are the model's."""
    o = run(MODEL_CASE)
    assert not o["model_infos"], o["model_infos"][:3]
    assert not o["model_bad"], o["model_bad"][:5]


@pytest.mark.parametrize("case", ["R5", "ring"])
def test_keep_volatile(case):
    """6.  RAFT_REPLAY_KEEP_VOLATILE: role, commitIndex, flags, timers and
    sessions are a fresh engine's still; the persistent words are B7's."""
    o = run(case)
    R, W = o["R"], o["W"]
    (sk, lk), (sb, lb), fresh = o["keep"], o["B7"], o["fresh"]
    for r in range(R):
        for name in ("role", "commit", "election_ms", "flags", "phase_ms", "retry_ms"):
            assert np.array_equal(fld(sk, R, r, name), fld(fresh, R, r, name)), (r, name)
        for name in ("term", "voted", "last", "phys"):
            assert np.array_equal(fld(sk, R, r, name), fld(sb, R, r, name)), (r, name)
    assert np.array_equal(sk[:, R * NF:], fresh[:, R * NF:])
    same_logs(sb, lb, lk, R, W, f"{case} keep_volatile")


def test_amnesia_recovery_equals_the_host_recover():
    """3.  RAFT_RESTART_AMNESIA of chosen replicas, then recover_on_device: the
    engine equals a twin that took the host recover of the same nodes, field
    by field, log by log and in its digest; both step on with equal counters,
    and the audit stays clean."""
    kw = CASES["R5"]
    R = 5
    rng = np.random.default_rng(3)
    mask = rng.integers(0, 32, G, dtype=np.uint8)
    mask[::7] = 0                                                          # groups left alone
    mask[3::11] = 31                                                       # groups that lose every replica
    nodes = [(g, r) for g in range(G) for r in range(R) if mask[g] >> r & 1]
    with RaftEngine(abi.make_params(**kw)) as e, RaftEngine(abi.make_params(**kw)) as twin:
        svcs = [svc_mod.RaftService(e), svc_mod.RaftService(twin)]
        for x, svc in zip((e, twin), svcs):
            x.step(200, counters=False)
            svc.persist()
            x.step(100, counters=False)
            tot = svc.persist(max_records=1000)
            assert tot["entries"] > 0 and tot["lost"] == 0
            info = x.restart(mask, amnesia=True)
            assert info["restarted"] == len(nodes) and info["entries_dropped"] > 0
        assert svcs[0].wal_image.length.max() > 256 + 2                    # a run over a workgroup boundary
        info = svcs[0].recover_on_device(nodes + nodes[:3])                # (a node named twice counts once)
        lengths = sum(int(svcs[0].wal_image.length[g, r]) for g, r in nodes)
        assert info == dict(applied=lengths + 2 * len(nodes), replicas=len(nodes), hardstates=len(nodes),
                            truncates=len(nodes), entries=lengths, malformed=0)
        for g, r in nodes:
            svcs[1].recover(g, r)
        (st, (t, c)), (ts, (tt, tc)) = snapshot(e), snapshot(twin)
        same_replica_words(st, ts, R, "recover", skip=())
        assert np.array_equal(st, ts) and np.array_equal(t, tt) and np.array_equal(c, tc)
        assert e.digest() == twin.digest()
        audit = e.audit()
        audit.observe()
        for k in range(10):
            ce, ct = e.step(10)[:, : abi.NUM_COUNTERS], twin.step(10)[:, : abi.NUM_COUNTERS]
            assert np.array_equal(ce, ct), f"steps {10 * k}..: counters differ from the host-recovered twin"
            assert audit.observe()["flagged"] == 0
        assert e.digest() == twin.digest()


def crafted_engine(ring):
    e = RaftEngine(abi.make_params(R=RP.CRAFT_R, G=RP.CRAFT_G, log_cap=RP.CRAFT_CAP,
                                   log_window=RP.CRAFT_W if ring else 0))
    st, t, c = RP.crafted()
    e.write_state(st)
    e.write_log(t, c)
    e.step_index = 40
    return e, st, t, c


@pytest.mark.parametrize("ring", [False, True], ids=["flat", "ring"])
def test_malformed_batches_are_refused_whole(ring):
    """5.  One batch per malformed rule: RAFT_EINVAL, malformed as the model
    counts, state and logs byte-identical before and after.  The well-formed
    batch beside them leaves what the model leaves."""
    e, st, t, c = crafted_engine(ring)
    W = RP.CRAFT_W if ring else 0
    with e:
        before = (e.read_state().tobytes(), *(a.tobytes() for a in e.read_log()))
        for name, (rec, count) in RP.malformed_batches(ring).items():
            want = RP.replay_into(e, rec, st.copy(), t.copy(), c.copy())
            assert want["malformed"] == count, name
            with pytest.raises(RaftError, match=r"\(-1\).*malformed") as err:
                rpl.replay(e, rec)
            assert err.value.info == want, (name, err.value.info)
            assert (e.read_state().tobytes(), *(a.tobytes() for a in e.read_log())) == before, name
        import torch
        rec, count = RP.malformed_batches(ring)["several at once"]
        dev = torch.from_numpy(rec.view(np.uint8).copy()).to("cuda:0")
        torch.cuda.synchronize()
        with pytest.raises(RaftError, match="malformed") as err:
            rpl.replay_dev(e, dev.data_ptr(), len(rec))
        assert err.value.info["malformed"] == count
        assert (e.read_state().tobytes(), *(a.tobytes() for a in e.read_log())) == before
        good = RP.good_batch(ring)
        want = RP.replay_into(e, good, st, t, c)
        assert rpl.replay(e, good) == want and want["malformed"] == 0
        got, (gt, gc) = snapshot(e)
        assert np.array_equal(got, st)
        if ring:                # the ring held entries 4..7 only: a TRUNCATE uncovers slots below them that it never had
            for a in (t, c, gt, gc):
                a[:, :, :RP.CRAFT_CAP // 2 - W] = 0
        assert not RP.persistent_errors(got, gt, gc, st, t, c, RP.CRAFT_R, RP.CRAFT_CAP, W)
        # and the engine steps on from what the replay left (the tail cache of every touched replica is in use)
        e.step(5)


def test_argument_checks():
    e, st, t, c = crafted_engine(False)
    lib = rpl.bind()
    with e:
        before = e.read_state().tobytes()
        zero = dict.fromkeys(RP.INFO_KEYS, 0)
        assert rpl.replay(e, np.zeros(0, abi.WAL_RECORD_DTYPE)) == zero and rpl.replay_dev(e, 0, 0) == zero
        good = RP.good_batch()
        info = rpl.raft_replay_info()
        p = C.c_void_p(good.ctypes.data)
        for args, why in (((p, -1, 0, C.byref(info)), "negative"), ((p, 1 << 31, 0, C.byref(info)), "2\\^31"),
                          ((None, 3, 0, C.byref(info)), "null buffer"), ((p, 3, 2, C.byref(info)), "flag"),
                          ((p, 3, 0, None), "null info")):
            for fn in (lib.raft_wal_replay, lib.raft_wal_replay_dev):
                assert fn(e._h, *args) == abi.RAFT_EINVAL
                assert re.search(why, lib.raft_last_error().decode()), (why, lib.raft_last_error())
        assert lib.raft_wal_replay_dev(e._h, C.c_void_p(good.ctypes.data + 4), 1, 0, C.byref(info)) == abi.RAFT_EINVAL
        assert b"8-byte aligned" in lib.raft_last_error()
        with pytest.raises(ValueError):
            rpl.replay_dev(e, good.ctypes.data + 4, 1)
        with pytest.raises(ValueError):
            rpl.replay_dev(e, 0, 3)
        with pytest.raises(ValueError):
            rpl.replay(e, np.zeros(3, np.int32))
        assert e.read_state().tobytes() == before


def test_standby_follows_the_source():
    """RaftService.standby: a never-stepped engine fed by poll and
    keep_volatile replays holds the source's persistent state after each call."""
    kw = dict(CASES["R5"], G=16)
    with RaftEngine(abi.make_params(**kw)) as a, RaftEngine(abi.make_params(**kw)) as b:
        sa, sb = svc_mod.RaftService(a), svc_mod.RaftService(b)
        for k in range(3):
            a.step(40, counters=False)
            tot = sa.standby(sb, max_records=500)
            assert tot["applied"] > 0 and tot["lost"] == 0 and (k > 0 or tot["polls"] > 1)
            (st, (t, c)), (bs, (bt, bc)) = snapshot(a), snapshot(b)
            assert not RP.persistent_errors(bs, bt, bc, st, t, c, 5, CAP)
        assert not any(fld(bs, 5, r, "role").any() or fld(bs, 5, r, "commit").any() for r in range(5))
