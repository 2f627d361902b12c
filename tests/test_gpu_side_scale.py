"""The side-path kernels at 20,011 groups of five (marker `gpu`): past the 64
stripes of the striped totals several times over, past one block of rocprim's
scan, past one digit and one block of its radix sort, on sub-ranges that start
far from group 0 and inside a wave.  Each call is judged three ways: its info
in closed form (numpy over the image written), everything numpy can express in
full, and the plain-Python models on the groups side_scale_model.slice_groups
names (in full where that is cheap).  Every comparison is exact."""
import importlib

import numpy as np
import pytest

import apply_model as AM
import client_model as CM
import nemesis_model as NM
import noop_model as NO
import oracle as O
import restart_model as RM
import side_scale_model as S
import sm_model as SM
from helpers import abi, assert_same_logs, assert_same_state, blank_groups, masked_logs, set_fld

pytestmark = pytest.mark.gpu

RaftEngine = importlib.import_module("raft-kotlin_amd.engine").RaftEngine

R, G = 5, 20_011
SUB = (4_099, 12_345)                     # a sub-range that starts inside a wave of either shape, 64 waves in
SEED = 20_011

# the sizes are the point of this file: if someone changes G, fail here instead
# of silently falling back inside one stripe pass, one scan block or one sort digit
for _R in (5, 3):
    assert all(v > 2 * S.HDR_STRIPES for v in S.waves(G, _R).values()), S.waves(G, _R)
    assert all(v > 2 * S.HDR_STRIPES for v in S.waves(SUB[1], _R).values())
    assert G * _R + 1 > 4 * max(S.SCAN_BLOCKS)                         # the drain's scan items
    assert SUB[0] % (64 // _R) != 0 and SUB[0] // (64 // _R) > S.HDR_STRIPES
GPW = 64 // R
assert G * R == 100_055 and -(-G * R // 64) == 1_564 and -(-G // GPW) == 1_668 and -(-G // 64) == 313
assert (G * R + 1) // max(S.SCAN_BLOCKS) >= 26
assert (G - 1).bit_length() == 15 and G > 4 * S.BLOCK
assert SUB[0] + SUB[1] < G and (G * R) % 64 != 0 and G % GPW != 0 and G % 64 != 0


def untouched(before: dict, after: dict, sel, label=""):
    """Nothing outside the groups `sel` moved: every array of `before` ([G, ...])
    equals its twin in `after` over the complement of the selection."""
    keep = S.complement(len(next(iter(before.values()))), sel)
    for k, b in before.items():
        assert np.array_equal(b[keep], after[k][keep]), f"{label}: {k} moved outside the selection"


def on_slices(n, kind, Rr, g0=0):
    """The groups the Python models run on (side_scale_model.slice_groups, seed fixed here)."""
    return S.slice_groups(n, kind, Rr, SEED, g0).tolist()


def same(got, want, label):
    if len(got) != len(want) or not np.array_equal(got, want):
        k = min(len(got), len(want))
        bad = np.flatnonzero(got[:k] != want[:k])
        at = int(bad[0]) if len(bad) else k
        raise AssertionError(f"{label}: {len(got)} vs {len(want)} records; first difference at {at}: "
                             f"{got[at] if at < len(got) else None} vs {want[at] if at < len(want) else None}")


def image(e, Rr):
    """Everything a side path may write, the log slots at or beyond physLen (unspecified) zeroed."""
    st = e.read_state()
    t, c = masked_logs(st, *e.read_log(), Rr)
    out = dict(state=st, terms=t, cmds=c, applied=e.applied())
    if e.sm_slots:
        out["heads"], out["regs"] = e.sm_read()
    return out


# ---- 1. the drain ----
def test_drain():
    cap = 8
    w, t, c, lens = S.committed_image(G, R, cap)
    zero = np.zeros((G, R), np.int32)
    whole = S.drain_stream(t, c, zero, lens)
    total = int(lens.sum())
    first = np.cumsum(lens.ravel()) - lens.ravel()
    assert lens.ravel()[4_000] >= 2
    inside = int(first[4_000]) + 1                                     # inside the run of scan item 4,000: the second block
    assert max(S.SCAN_BLOCKS) < 4_000 < 2 * min(S.SCAN_BLOCKS)
    with RaftEngine(abi.make_params(R=R, G=G, log_cap=cap)) as e:
        e.write_state(w)
        e.write_log(t, c)
        assert e.peek_committed() == dict(delivered=0, pending=total, lost=0, regressed=0, status=0)
        got, info = e.drain_committed()
        assert info == dict(delivered=total, pending=0, lost=0, regressed=0, status=0)
        same(got, whole, "the whole stream")
        assert np.array_equal(e.applied(), lens)
        zs = np.zeros((G, R), np.int64)
        for g in on_slices(G, "scan", R):
            want, _ = AM.drain(w, t, c, zs, R, cap, g0=g, n=1, peek=False)
            zs[g] = 0
            same(got[got["group"] == g], want, f"group {g} against the model")
        for cut in (total - 3, inside):
            e.set_applied(zero)
            got, info = e.drain_committed(max_entries=cut)
            assert info == dict(delivered=cut, pending=total - cut, lost=0, regressed=0, status=0)
            same(got, whole[:cut], f"cut at {cut}")
            want_applied = np.clip(cut - first, 0, lens.ravel()).reshape(G, R)
            assert np.array_equal(e.applied(), want_applied), f"lastApplied after a cut at {cut}"
            rest, info = e.drain_committed()
            assert info == dict(delivered=total - cut, pending=0, lost=0, regressed=0, status=0)
            same(rest, whole[cut:], f"the rest after {cut}")
            assert np.array_equal(e.applied(), lens)
        e.set_applied(zero)
        got, info = e.drain_committed(replica=2)                      # the other branch of sel_idx
        same(got, whole[whole["replica"] == 2], "replica 2")
        assert info["delivered"] == int(lens[:, 2].sum()) and info["pending"] == 0
        only2 = np.zeros_like(lens)
        only2[:, 2] = lens[:, 2]
        assert np.array_equal(e.applied(), only2)
        e.set_applied(zero)
        g0, n = SUB
        got, info = e.drain_committed(g0, n)
        same(got, S.drain_stream(t, c, zero, lens, g0, n), "the sub-range")
        assert info == dict(delivered=int(lens[g0:g0 + n].sum()), pending=0, lost=0, regressed=0, status=0)
        sub = np.zeros_like(lens)
        sub[g0:g0 + n] = lens[g0:g0 + n]
        assert np.array_equal(e.applied(), sub)
        assert np.array_equal(e.read_state(), w)                       # a drain writes lastApplied and nothing else
        assert_same_logs(w, e.read_log(), (t, c), R, "the logs after the drains")


# ---- 2. the machine ----
@pytest.mark.parametrize("Rr", [5, 3])
def test_machine(Rr):
    cap, slots = 8, 8
    w, t, c, lens = S.committed_image(G, Rr, cap)
    gi = np.arange(G)
    for r in range(Rr):                                                # a leader in most groups, none in every 11th
        set_fld(w, Rr, r, "role", np.where((gi % Rr == r) & (gi % 11 != 0), abi.LEADER, abi.FOLLOWER))
    zero = np.zeros_like(lens)
    g0, n = SUB
    with RaftEngine(abi.make_params(R=Rr, G=G, log_cap=cap)) as e, RaftEngine(abi.make_params(R=Rr, G=G, log_cap=cap)) as s:
        for x in (e, s):
            x.write_state(w)
            x.write_log(t, c)
            x.sm_configure(slots)
        info = e.sm_apply()
        assert info == dict(applied=S.apply_total(lens, zero), lost=0, regressed=0, status=0)
        h, regs = e.sm_read()
        assert np.array_equal(h["applied"], lens) and not h["lost"].any()
        assert np.array_equal(h["hash"] != 0, lens > 0)
        info = s.sm_apply(g0, n)
        assert info == dict(applied=S.apply_total(lens, zero, g0, n), lost=0, regressed=0, status=0)
        hs, rs = s.sm_read()
        sub = np.zeros_like(lens)
        sub[g0:g0 + n] = lens[g0:g0 + n]
        assert np.array_equal(hs["applied"], sub)
        blank = dict(heads=np.zeros_like(hs), regs=np.zeros_like(rs))
        untouched(blank, dict(heads=hs, regs=rs), np.arange(g0, g0 + n), "sub-range apply")
        assert np.array_equal(hs[g0:g0 + n], h[g0:g0 + n]) and np.array_equal(rs[g0:g0 + n], regs[g0:g0 + n])
        mach = SM.Machine(G, Rr, slots)
        # sm_apply_kernel is a tile kernel: a wave owns 64 replicas of the selection, counted from g0
        for g in sorted(set(on_slices(G, "tile", Rr) + on_slices(n, "tile", Rr, g0) + on_slices(G, "scan", Rr))):
            SM.apply(w, t, c, mach, Rr, cap, g0=g, n=1)
            want = mach.heads(g, 1)[0]
            assert np.array_equal(h[g], want), f"heads of group {g}: {h[g]} vs {want}"
            assert np.array_equal(regs[g], mach.reg[g]), f"registers of group {g}"
        assert e.sm_apply() == dict(applied=0, lost=0, regressed=0, status=0)
        # State Machine Safety: no two replicas of a group share a length, so nothing is flagged...
        assert e.sm_check(flags=True)[0] == 0
        bad = np.arange(0, G, 997)                                     # ...until replica 0 takes replica 1's with another hash
        h2 = h.copy()
        h2["applied"][bad, 0] = h["applied"][bad, 1]
        h2["hash"][bad, 0] = h["hash"][bad, 1] ^ np.uint64(1 << 40)
        e.sm_write(heads=h2)
        cnt, flags = e.sm_check(flags=True)
        want = np.zeros(G, np.uint8)
        want[bad] = 1
        assert np.array_equal(flags, want) and cnt == len(bad) and np.array_equal(S.sm_check_expect(h2), want)
        cnt, flags = e.sm_check(g0, n, flags=True)
        assert np.array_equal(flags, want[g0:g0 + n]) and cnt == int(want[g0:g0 + n].sum())
        # the batched read
        rng = np.random.default_rng(SEED)
        m = 50_003
        groups = rng.integers(0, G, m)
        groups[:4] = (0, G - 1, 0, G - 1)
        keys = rng.integers(0, 2 ** 32, m, dtype=np.uint32)
        assert np.array_equal(S.lowest_leader(w, Rr), CM.leaders(w, Rr)["leader"])
        for reps in (np.full(m, -1), rng.integers(0, Rr, m), rng.integers(-1, Rr, m)):
            got = e.sm_get(groups, keys, reps)
            want = S.sm_get_expect(w, h2, regs, Rr, groups, keys, reps)
            same(got, want, "sm_get")
        assert (got["replica"] == -1).any() and got["value"].any()
        assert np.array_equal(e.read_state(), w)


# ---- 3. leaders, propose, resolve ----
@pytest.mark.parametrize("mode", [0, 1], ids=["reference", "textbook"])
def test_client(mode):
    cap = 32
    kw = dict(R=R, G=G, log_cap=cap, mode=mode)
    w, t, c = S.led_image(G, R, cap)
    rng = np.random.default_rng(SEED + mode)
    m = 100_003
    hot = 12_345
    groups = rng.integers(0, G, m, dtype=np.int64)
    groups[rng.choice(m, 3_000, replace=False)] = hot                  # a run spanning many workgroups of the sorted batch
    groups[:2] = (0, G - 1)
    cmds = rng.integers(1, 2 ** 32, m, dtype=np.uint32)
    assert CM.leaders(w, R)["leader"][hot] >= 0
    o = O.Oracle(abi.make_params(**kw))
    with RaftEngine(abi.make_params(**kw)) as e:
        for x in (e, o):
            x.write_state(w)
            x.write_log(t, c)
        ld = e.leaders()
        same(ld, CM.leaders(w, R), "leaders")
        same(e.leaders(*SUB), ld[SUB[0]:SUB[0] + SUB[1]], "leaders of the sub-range")
        assert (ld["leader"] < 0).any() and (ld["n_leaders"] == 2).any()
        want, rc = CM.propose(o, groups, cmds, textbook=bool(mode))
        got = e.propose(groups, cmds)
        same(got, want, "tickets")
        assert e.last_status == rc
        for st in (CM.ACCEPTED, CM.NO_LEADER, CM.LOG_FULL):
            assert (got["status"] == st).any(), st
        at_hot = got[groups == hot]
        acc = at_hot[at_hot["status"] == CM.ACCEPTED]
        assert len(at_hot) >= 3_000 and np.all(np.diff(acc["index"]) == 1)     # batch order inside the run
        st, logs = e.read_state(), e.read_log()
        assert_same_state(st, o.read_state(), R, "after the batch")
        assert_same_logs(st, logs, o.read_log(), R, "after the batch")
        # the leaders of every fourth group commit all they hold: those tickets resolve COMMITTED
        gi = np.arange(G)
        for r in range(R):
            at = (ld["leader"] == r) & (gi % 4 == 2)
            st[at, r * abi.NUM_FIELDS + abi.F_INDEX["commit"]] = st[at, r * abi.NUM_FIELDS + abi.F_INDEX["last"]]
        # ...and in another fourth the leader's slot was overwritten in a later term: those are LOST
        acc = got["status"] == CM.ACCEPTED
        gone = acc & (groups % 4 == 3)
        logs[0][groups[gone], got["replica"][gone], got["index"][gone]] = 99
        e.write_state(st)
        e.write_log(*logs)
        res = e.resolve(groups, got, cmds)
        wres, wrc = CM.resolve(st, *logs, groups, got, cmds, R, cap)
        same(res, wres, "resolve")
        assert e.last_status == wrc
        for s_ in (CM.NONE, CM.PENDING, CM.COMMITTED, CM.LOST):
            assert (res["status"] == s_).any(), s_
    o.close()


def test_client_sixteen_bit_keys():
    """G = 65,536: the sort key is exactly 16 bits wide; one batch addresses
    the first and the last group."""
    G2, cap = 65_536, 8
    assert (G2 - 1).bit_length() == 16 and G2 & (G2 - 1) == 0
    kw = dict(R=R, G=G2, log_cap=cap)
    w = blank_groups(G2, R)
    gi = np.arange(G2)
    for r in range(R):
        set_fld(w, R, r, "term", 3)
        set_fld(w, R, r, "role", np.where(gi % R == r, abi.LEADER, abi.FOLLOWER))
    rng = np.random.default_rng(SEED)
    groups = rng.integers(1, G2 - 1, 5_003, dtype=np.int64)
    groups[[0, 1, 2, 5_000, 5_001, 5_002]] = (G2 - 1, 0, G2 - 1, 0, G2 - 1, 0)
    cmds = rng.integers(1, 2 ** 32, len(groups), dtype=np.uint32)
    o = O.Oracle(abi.make_params(**kw))
    with RaftEngine(abi.make_params(**kw)) as e:
        for x in (e, o):
            x.write_state(w)
        want, rc = CM.propose(o, groups, cmds)
        got = e.propose(groups, cmds)
        same(got, want, "tickets")
        assert list(got["index"][[0, 2, 5_001]]) == [0, 1, 2] and list(got["index"][[1, 5_000, 5_002]]) == [0, 1, 2]
        st = e.read_state()
        assert_same_state(st, o.read_state(), R, "after the batch")
        assert_same_logs(st, e.read_log(), o.read_log(), R, "after the batch")
    o.close()


# ---- 6. no-op entries ----
def test_noops():
    cap, cmd = 16, NO.NOOP
    kw = dict(R=R, G=G, log_cap=cap, mode=abi.MODE_TEXTBOOK)
    w, t, c = S.led_image(G, R, cap)
    o = O.Oracle(abi.make_params(**kw))
    with RaftEngine(abi.make_params(**kw)) as e:
        for x in (e, o):
            x.write_state(w)
            x.write_log(t, c)
        for call in range(2):
            st0, (t0, _) = o.read_state(), o.read_log()
            closed = S.noop_totals(st0, t0, R, cap, True)
            winfo, wtk, wcmd, rc = NO.append_noops(o, 0, G, cmd, textbook=True)
            info, tk, tc = e.append_noops(cmd=cmd, tickets=True)
            assert info == winfo == closed, f"call {call}: {info} vs {winfo} vs {closed}"
            assert e.last_status == rc
            same(tk, wtk, f"tickets of call {call}")
            assert np.array_equal(tc, wcmd)
            st, logs = e.read_state(), e.read_log()
            assert_same_state(st, o.read_state(), R, f"call {call}")
            assert_same_logs(st, logs, o.read_log(), R, f"call {call}")
            if call == 0:
                first = info
                assert info["appended"] > G // 2 and info["current"] > 0 and info["no_leader"] > 0
            else:
                assert info["appended"] == 0 and info["current"] == first["current"] + first["appended"]
        # a sub-range on a twin: nothing outside it moves
        g0, n = SUB
        with RaftEngine(abi.make_params(**kw)) as s:
            s.write_state(w)
            s.write_log(t, c)
            before = image(s, R)
            info = s.append_noops(g0, n, cmd=cmd)
            assert info == S.noop_totals(w, t, R, cap, True, g0, n)
            after = image(s, R)
            untouched(before, after, np.arange(g0, g0 + n), "sub-range no-ops")
            assert np.array_equal(after["state"][g0:g0 + n], st[g0:g0 + n])      # what the whole-range call left there
    o.close()


# ---- 7. restart ----
def restart_image(cap=16, slots=8):
    w, t, c = S.led_image(G, R, cap)
    for r in range(R):
        set_fld(w, R, r, "retry_ms", 7)                                # every restart changes its replica's image
        set_fld(w, R, r, "phase_ms", 3)
    rng = np.random.default_rng(SEED)
    heads = np.zeros((G, R), abi.SM_HEAD_DTYPE)
    heads["applied"] = rng.integers(1, cap, (G, R))
    heads["hash"] = rng.integers(1, 2 ** 63, (G, R), dtype=np.uint64)
    regs = rng.integers(1, 2 ** 32, (G, R, slots), dtype=np.uint32)
    applied = rng.integers(1, cap, (G, R)).astype(np.int32)
    return w, t, c, heads, regs, applied


def load_restart(e, img, slots=8):
    w, t, c, heads, regs, applied = img
    e.write_state(w)
    e.write_log(t, c)
    e.sm_configure(slots)
    e.sm_write(heads, regs)
    e.set_applied(applied)


def model_restart(e, img, sel, g0, flags, down_steps):
    """restart_model.restart of groups [g0, g0 + len(sel)) of the image: (info, the image after)."""
    w, t, c, heads, regs, applied = (a.copy() for a in img)
    n = len(sel)
    info = RM.restart(w[g0:g0 + n], sel, R=R, seed=int(e.p.seed), step=int(e.step_index), gid0=int(e.p.g0) + g0,
                      emin=int(e.p.election_min_ms), emax=int(e.p.election_max_ms), flags=flags, down_steps=down_steps,
                      applied=applied[g0:g0 + n], heads=heads[g0:g0 + n], regs=regs[g0:g0 + n])
    t, c = masked_logs(w, t, c, R)
    return info, dict(state=w, terms=t, cmds=c, applied=applied, heads=heads, regs=regs)


@pytest.mark.parametrize("flags", [0, RM.REPLAY, RM.AMNESIA], ids=["persistent", "replay", "amnesia"])
def test_restart_masks(flags):
    """The mask form, from the host over the whole range and from the device
    over the sub-range: about one replica in 50, every replica of each 997th
    group, down_steps 3.  The model runs over the whole range."""
    import torch
    img = restart_image()
    kwf = dict(amnesia=bool(flags & RM.AMNESIA), replay=bool(flags & RM.REPLAY), down_steps=3)
    with RaftEngine(abi.make_params(R=R, G=G, log_cap=16, seed=5)) as e:
        for g0, n, dev in ((0, G, False), (*SUB, True)):
            load_restart(e, img)
            mask = S.sparse_mask(n, R, SEED + dev)
            sel = RM.select_mask(mask, R)
            assert (sel.reshape(-1)[: n * R // 60 * 60].reshape(-1, 60).sum(1) > 1).any()    # several in one wave
            if dev:
                dm = torch.from_numpy(mask).to("cuda:0")
                torch.cuda.synchronize()
                info = e.restart_dev(dm.data_ptr(), g0=g0, n=n, **kwf)
            else:
                info = e.restart(mask, g0=g0, n=n, **kwf)
            closed = S.restart_totals(img[0][g0:g0 + n], sel, R, bool(flags & RM.AMNESIA))
            winfo, want = model_restart(e, img, sel, g0, flags, 3)
            assert info == closed == winfo, f"{info} vs {closed} vs {winfo}"
            assert info["leaders"] > 0 and info["restarted"] > n * R // 60
            got = image(e, R)
            before = dict(zip(("state", "terms", "cmds", "heads", "regs", "applied"), img))
            before["terms"], before["cmds"] = masked_logs(*img[:3], R)
            untouched(before, got, np.arange(g0, g0 + n)[sel.any(1)], "restart")
            assert_same_state(got["state"], want["state"], R, f"restart flags {flags} dev {dev}")
            for k in ("terms", "cmds", "applied", "heads", "regs"):
                assert np.array_equal(got[k], want[k]), f"restart flags {flags} dev {dev}: {k}"


@pytest.mark.parametrize("flags", [0, RM.REPLAY, RM.AMNESIA], ids=["persistent", "replay", "amnesia"])
def test_restart_random(flags):
    """restart_random at 20,000 ppm over the sub-range.  The model draws Philox
    in Python, so it runs on the slices; every restart zeroes the replica's
    retryMs (7 in the image), which counts the restarted replicas in full."""
    img = restart_image()
    g0, n = SUB
    ppm = 20_000
    with RaftEngine(abi.make_params(R=R, G=G, log_cap=16, seed=5)) as e:
        load_restart(e, img)
        e.step_index = 9
        info = e.restart(ppm=ppm, g0=g0, n=n, amnesia=bool(flags & RM.AMNESIA), replay=bool(flags & RM.REPLAY))
        got = image(e, R)
        was = S.cols(img[0], R, "retry_ms")
        now = S.cols(got["state"], R, "retry_ms")
        # [G, R]: the replicas that restarted, read from the after image: outside the slices the totals
        # below are a consistency condition on the kernel's own selection, not an independent draw
        hit = now != was
        assert not hit[:g0].any() and not hit[g0 + n:].any()
        closed = S.restart_totals(img[0], hit, R, bool(flags & RM.AMNESIA))
        assert info == closed, f"{info} vs {closed}"
        assert n * R * ppm // 1_000_000 // 2 < info["restarted"] < n * R * ppm // 1_000_000 * 2
        before = dict(zip(("state", "terms", "cmds", "heads", "regs", "applied"), img))
        before["terms"], before["cmds"] = masked_logs(*img[:3], R)
        untouched(before, got, np.flatnonzero(hit.any(1)), "restart_random")
        sl = on_slices(n, "gpw", R, g0)
        inside = 0
        for g in sl:
            sel = RM.select_random(int(e.p.seed), 9, int(e.p.g0) + g, 1, R, ppm)
            assert np.array_equal(sel[0], hit[g]), f"group {g}: the selection"
            inside += int(sel.sum())
            w1 = img[0][g:g + 1].copy()
            a1, h1, r1 = img[5][g:g + 1].copy(), img[3][g:g + 1].copy(), img[4][g:g + 1].copy()
            RM.restart(w1, sel, R=R, seed=int(e.p.seed), step=9, gid0=int(e.p.g0) + g,
                       emin=int(e.p.election_min_ms), emax=int(e.p.election_max_ms), flags=flags,
                       applied=a1, heads=h1, regs=r1)
            assert_same_state(got["state"][g:g + 1], w1, R, f"group {g}")
            assert np.array_equal(got["applied"][g], a1[0]) and np.array_equal(got["heads"][g], h1[0])
            assert np.array_equal(got["regs"][g], r1[0])
        outside = int(hit[S.complement(G, sl)].sum())
        assert inside + outside == info["restarted"]


# ---- 9. isolate, heal, list ----
def test_nemesis():
    cap = 8
    w, t, c = S.led_image(G, R, cap)
    groups, targets, steps = NM.contended_batch(G, 5, 50_003)
    with RaftEngine(abi.make_params(R=R, G=G, log_cap=cap)) as e:
        e.write_state(w)
        e.write_log(t, c)
        model = w.copy()
        for replace in (False, True):
            want, rc = NM.isolate(model, groups, targets, steps, R, replace)
            got = e.isolate(groups, targets, steps, replace=replace)
            assert rc == abi.RAFT_OK
            same(got, want, f"tickets, replace {replace}")
            assert_same_state(e.read_state(), model, R, f"isolate, replace {replace}")
            seen = set(got["status"].tolist())
            assert {NM.SET, NM.NO_LEADER, NM.DUPLICATE, NM.INVALID} <= seen and (NM.BUSY in seen) == (not replace)
        g0, n = SUB
        mask = np.random.default_rng(SEED).integers(0, 32, n).astype(np.uint8)
        closed = S.heal_totals(model[g0:g0 + n, S.ISO], mask)
        winfo = NM.heal(model, R, mask, g0)
        info = e.heal_network(mask, g0)
        assert info == winfo == closed, f"{info} vs {winfo} vs {closed}"
        assert min(info.values()) > S.HDR_STRIPES
        st = e.read_state()
        assert_same_state(st, model, R, "heal")
        untouched(dict(state=w), dict(state=st), np.union1d(groups, np.arange(g0, g0 + n)), "isolate and heal")
        info, rec = e.isolated()
        winfo, wrec = S.isolated_expect(model, R)
        assert info == winfo and info["running"] > G // 4
        same(rec, wrec, "isolated")
        minfo, mrec = NM.list_isolated(model, R)
        assert info == minfo and np.array_equal(rec, mrec.astype(abi.ISOLATED_DTYPE))
        info, rec = e.isolated(g0, n, max_events=1_000)
        winfo, wrec = S.isolated_expect(model, R, g0, n, 1_000)
        assert info == winfo and info["pending"] > 0
        same(rec, wrec, "isolated, sub-range and cut")
        closed = S.heal_totals(model[:, S.ISO])
        assert e.heal_network() == closed and e.isolated(peek=True)[0]["running"] == 0
        assert_same_logs(st, e.read_log(), (t, c), R, "logs")


def test_isolated_past_one_scan_block():
    """300,001 groups of three: 4,688 wave counts to scan, more than one block
    of rocprim's scan; the order of the records holds across the boundary."""
    G3, R3, cap = 300_001, 3, 8
    assert -(-G3 // 64) > max(S.SCAN_BLOCKS) and G3 > 64 * max(S.SCAN_BLOCKS)
    groups = np.arange(0, G3, 7, dtype=np.int64)
    targets = (groups % R3).astype(np.int32)
    steps = (1 + groups % 30).astype(np.int32)
    model = blank_groups(G3, R3)
    model[groups, S.ISO] = steps << 8 | targets
    with RaftEngine(abi.make_params(R=R3, G=G3, log_cap=cap)) as e:
        e.write_state(blank_groups(G3, R3))
        tk = e.isolate(groups, targets, steps)
        assert np.all(tk["status"] == NM.SET) and np.array_equal(tk["replica"], targets) and not tk["prev"].any()
        assert np.array_equal(e.read_state(), model)
        winfo, whole = S.isolated_expect(model, R3)
        total = len(groups)
        info, rec = e.isolated()
        assert info == winfo == dict(delivered=total, pending=0, running=total)
        same(rec, whole, "isolated")
        assert np.array_equal(rec["group"], groups)
        assert (rec["group"] < 64 * min(S.SCAN_BLOCKS)).any() and (rec["group"] >= 64 * max(S.SCAN_BLOCKS)).any()
        for cut in (total - 7, 10_000):                                # in the last scan block, and in the first
            assert cut == total - 7 or whole["group"][cut] < 64 * min(S.SCAN_BLOCKS)
            info, rec = e.isolated(max_events=cut)
            assert info == dict(delivered=cut, pending=total - cut, running=total)
            same(rec, whole[:cut], f"cut at {cut}")
        g0, n = 64 * max(S.SCAN_BLOCKS) - 100, 50_000                   # a sub-range across the block's end
        info, rec = e.isolated(g0, n)
        winfo, wrec = S.isolated_expect(model, R3, g0, n)
        assert info == winfo
        same(rec, wrec, "sub-range")


# ---- 4. the ReadIndex pair ----
def test_reads():
    import read_model as RD
    cap, slots = 8, 8
    kw = dict(R=R, G=G, log_cap=cap, mode=abi.MODE_TEXTBOOK)
    w, t, c = S.settled_image(G, R, cap)
    gi = np.arange(G)
    rng = np.random.default_rng(SEED)
    m = 100_003
    groups = rng.integers(0, G, m, dtype=np.int64)
    groups[:2] = (0, G - 1)
    keys = rng.integers(0, 2 ** 32, m, dtype=np.uint32)
    pick = np.unique(np.concatenate([[0, m - 1, 255, 256], rng.choice(m, 4_000, replace=False)]))
    with RaftEngine(abi.make_params(**kw)) as e:
        e.write_state(w)
        e.write_log(t, c)
        e.sm_configure(slots)
        assert e.sm_apply()["applied"] == int(S.cols(w, R, "commit").sum())
        tk = e.begin_reads(groups)
        want, rc = RD.begin(w, t, groups[pick], R, cap)
        same(tk[pick], want, "read tickets")
        assert e.last_status == rc == abi.RAFT_OK
        # in full: the ticket is a function of the group
        L = S.newest_leader(w, R)
        assert np.array_equal(tk["replica"], L[groups])
        assert np.array_equal(tk["status"] == RD.NO_LEADER, L[groups] < 0)
        assert np.array_equal(tk["status"] == RD.TERM_UNCOMMITTED, (L[groups] >= 0) & (groups % 5 == 0))
        assert np.array_equal(tk["read_index"], np.where(L[groups] >= 0, 4, -1))
        for st_ in (RD.ISSUED, RD.TERM_UNCOMMITTED, RD.NO_LEADER):
            assert (tk["status"] == st_).any(), st_
        # between begin and serve: a deposed leader, a lost quorum, a machine behind, a machine with a gap
        w2 = w.copy()
        heads, regs = e.sm_read()
        for r in range(R):
            set_fld(w2, R, r, "role", np.where((gi % 7 == 1), abi.FOLLOWER, S.cols(w, R, "role")[:, r]))
            set_fld(w2, R, r, "term", np.where((gi % 7 == 2) & (gi % R != r), 8, S.cols(w, R, "term")[:, r]))
        heads["applied"][gi % 7 == 3] = 1
        heads["lost"][gi % 7 == 4] = 1
        e.write_state(w2)
        e.sm_write(heads=heads)
        res = e.serve_reads(groups, tk, keys, check=False)             # a NO_LEADER ticket names no replica: INVALID
        wres, rc = RD.serve(w2, heads, regs, groups[pick], tk[pick], keys[pick], R, cap)
        same(res[pick], wres, "read results")
        assert e.last_status == rc == abi.RAFT_EINVAL
        for st_ in (RD.SERVED, RD.DEPOSED, RD.NO_QUORUM, RD.BEHIND, RD.GAPPED, RD.NONE, RD.INVALID):
            assert (res["status"] == st_).any(), st_
        ok = res["status"] == RD.SERVED                                # in full: the value of every served read
        assert np.array_equal(res["value"][ok], regs[groups[ok], tk["replica"][ok], keys[ok] & np.uint32(slots - 1)])
        assert np.array_equal(res["status"] == RD.NONE, tk["status"] == RD.TERM_UNCOMMITTED)
        assert np.array_equal(res["status"] == RD.INVALID, tk["status"] == RD.NO_LEADER)
        assert not res["value"][~ok].any()
        assert np.array_equal(e.read_state(), w2)


# ---- 5. transfer, resolve, evacuate ----
def test_transfers():
    import transfer_model as TM
    cap = 8
    w, t, c = S.settled_image(G, R, cap)
    lt = S.last_term_of(w, t, R)
    rng = np.random.default_rng(SEED)
    groups = np.concatenate([np.arange(G), rng.integers(0, G, 5_000)]).astype(np.int64)
    targets = rng.integers(-1, R + 1, len(groups)).astype(np.int32)    # AUTO, named, and R: INVALID
    targets[::2] = TM.AUTO
    with RaftEngine(abi.make_params(R=R, G=G, log_cap=cap)) as e, RaftEngine(abi.make_params(R=R, G=G, log_cap=cap)) as v:
        for x in (e, v):
            x.write_state(w)
            x.write_log(t, c)
        model = w.copy()
        want, rc = TM.transfer(model, groups, targets, R, lt)
        tk = e.transfer(groups, targets)
        same(tk, want, "transfer tickets")
        for st_ in (TM.SENT, TM.BEHIND, TM.BUSY, TM.UNREACHABLE, TM.SELF, TM.NO_LEADER, TM.INVALID):
            assert (tk["status"] == st_).any(), st_
        st = e.read_state()
        assert_same_state(st, model, R, "after the transfers")         # the electionMs words of the targets, nothing else
        assert (model != w).any(1).sum() > G // 2
        assert_same_logs(st, e.read_log(), (t, c), R, "transfer")
        # some targets have won (term 4), in some groups a third replica has (term 5)
        sent = tk[:G]["status"] == TM.SENT
        gi = np.arange(G)
        for r in range(R):
            won = sent & (tk[:G]["target"] == r) & (gi % 3 == 0)
            other = sent & ((tk[:G]["target"] + 1) % R == r) & (gi % 6 == 1)
            set_fld(model, R, r, "role", np.where(won | other, abi.LEADER, S.cols(model, R, "role")[:, r]))
            set_fld(model, R, r, "term", np.where(won, 4, np.where(other, 5, S.cols(model, R, "term")[:, r])))
        e.write_state(model)
        res = e.resolve_transfers(groups, tk)
        wres, rc = TM.resolve(model, groups, tk, R)
        same(res, wres, "resolve_transfers")
        for st_ in (TM.COMPLETED, TM.PENDING, TM.SUPERSEDED, TM.NONE):
            assert (res["status"] == st_).any(), st_
        # evacuate on the fresh twin, a mask per group of the sub-range
        g0, n = SUB
        mask = S.evacuate_mask(n, R, g0, SEED)
        model = w.copy()
        winfo = TM.evacuate(model, mask, R, g0, lt)
        closed = S.evacuate_totals(w, lt, mask, R, g0)
        info = v.evacuate(mask, g0)
        assert info == winfo == closed, f"{info} vs {winfo} vs {closed}"
        assert min(info.values()) > S.HDR_STRIPES, info
        st = v.read_state()
        assert_same_state(st, model, R, "after the evacuation")
        untouched(dict(state=w), dict(state=st), np.arange(g0, g0 + n), "evacuate")
        assert_same_logs(st, v.read_log(), (t, c), R, "evacuate")


# ---- 8. snapshot install ----
@pytest.mark.parametrize("W", [0, 16], ids=["flat", "ring16"])
@pytest.mark.parametrize("Rr", [5, 3])
def test_install(Rr, W):
    import snapshot_model as SN
    cap, slots = 32 if W else 8, 8
    kw = dict(R=Rr, G=G, log_cap=cap, mode=abi.MODE_TEXTBOOK, seed=5, **(dict(log_window=W) if W else {}))
    w, t, c = S.settled_image(G, Rr, cap)
    rng = np.random.default_rng(SEED + Rr)
    heads = np.zeros((G, Rr), abi.SM_HEAD_DTYPE)
    heads["applied"] = S.cols(w, Rr, "commit")
    heads["hash"] = rng.integers(1, 2 ** 63, (G, Rr), dtype=np.uint64)
    heads["lost"][::29] = 1                                            # a gapped machine: on the leader it bars the install
    regs = rng.integers(1, 2 ** 32, (G, Rr, slots), dtype=np.uint32)
    g0, n = SUB
    gi = np.arange(g0, g0 + n)
    mask = rng.integers(0, 1 << Rr, n).astype(np.uint8)
    mask |= np.where(gi % 3 == 0, 1 << (gi + 1) % Rr, 0).astype(np.uint8)       # the lagging replica of every third group
    sel = RM.select_mask(mask, Rr)
    with RaftEngine(abi.make_params(**kw)) as e:
        e.write_state(w)
        e.write_log(t, c)
        e.sm_configure(slots)
        e.sm_write(heads, regs)
        e.step_index = 9
        before = image(e, Rr)
        info = e.install_snapshot(mask, g0=g0)
        closed = S.install_totals(w[g0:g0 + n], heads[g0:g0 + n], sel, Rr, W)
        mw, mt, mc, mh, mr = (a[g0:g0 + n].copy() for a in (w, before["terms"], before["cmds"], heads, regs))
        winfo = SN.install(mw, mt, mc, mh, mr, sel, R=Rr, cap=cap, W=W, seed=int(e.p.seed), step=9,
                           gid0=int(e.p.g0) + g0, emin=int(e.p.election_min_ms), emax=int(e.p.election_max_ms))
        assert info == winfo == closed, f"{info} vs {winfo} vs {closed}"
        assert all(info[k] > S.HDR_STRIPES for k in SN.INFO_KEYS), info
        got = image(e, Rr)
        untouched(before, got, gi, "install")
        assert_same_state(got["state"][g0:g0 + n], mw, Rr, "install")
        mt, mc = masked_logs(mw, mt, mc, Rr)
        assert np.array_equal(got["terms"][g0:g0 + n], mt) and np.array_equal(got["cmds"][g0:g0 + n], mc)
        assert np.array_equal(got["heads"][g0:g0 + n], mh) and np.array_equal(got["regs"][g0:g0 + n], mr)
        again = e.install_snapshot(mask, g0=g0)                        # every installed replica is level now: copied again
        assert again == S.install_totals(mw, mh, sel, Rr, W), again
        assert again["installed"] == info["installed"] and again["ahead"] == info["ahead"]


# ---- 10. the outbox ----
def test_outbox():
    """20,003 records: 626 verdict tiles of 32 and a multi-block scan of their
    counts.  The same calls on the oracle's Host (outbox_model) and the engine."""
    import outbox_model as OM
    n = 20_003
    assert -(-n // 32) == 626 and -(-n // 32) > 2 * S.HDR_STRIPES and n > 4 * max(S.SCAN_BLOCKS)
    kw = S.outbox_kw(G)
    h = OM.Host(**kw)
    want = S.outbox_scenario(h, n, SEED)
    with RaftEngine(abi.make_params(**kw)) as e:
        got = S.outbox_scenario(e, n, SEED)
        S.outbox_closed(got, n)
        for k, ((info, done, rc, q), (winfo, wdone, wrc, wq)) in enumerate(zip(got, want)):
            assert info == winfo and rc == wrc, f"pump {k}: {info} vs {winfo}"
            assert done.dtype == abi.OUTBOX_DONE_DTYPE and q.dtype == abi.OUTBOX_ENTRY_DTYPE
            same(done, wdone, f"done records of pump {k}")
            same(q, wq, f"the queue after pump {k}")
        (a, _, _, _), (b, db, _, qb), (c, dc, _, qc) = got
        assert len(db) > 1_000 and b["deferred"] > 1_000 and b["retried"] > 0 and len(qc) > 0     # COMMITTED, retried, kept
        assert np.all(np.diff(db["tag"]) > 0) and np.all(np.diff(dc["tag"]) > 0) and np.all(np.diff(qc["tag"]) > 0)
        st = e.read_state()
        assert_same_state(st, h.read_state(), R, "after the pumps")
        assert_same_logs(st, e.read_log(), h.read_log(), R, "after the pumps")
    h.close()


# ---- 11. replay after a poll ----
def test_replay():
    """The WAL test's image with 600-entry rows in every 500th group: a run of
    601 records spans three 256-thread workgroups of both replay kernels."""
    import replay_model as RP
    rpl = importlib.import_module("raft-kotlin_amd.replay")
    RaftError = importlib.import_module("raft-kotlin_amd.engine").RaftError
    cap, piece = 600, 65_537
    w, t, c, lens = S.wal_image(G, R, cap)
    assert cap + 1 > 2 * S.BLOCK
    params = lambda: abi.make_params(R=R, G=G, log_cap=cap, seed=5)      # noqa: E731
    with RaftEngine(params()) as src, RaftEngine(params()) as whole, RaftEngine(params()) as parts:
        src.write_state(w)
        src.write_log(t, c)
        rec, pinfo = src.wal().poll()
        total = G * R + int(lens.sum())
        assert pinfo["delivered"] == len(rec) == total > 500_000 and pinfo["pending"] == 0
        same(rec, S.wal_stream(w, t, c, lens, R), "the polled stream")
        fresh = whole.read_state()
        # a malformed record in the middle: the whole batch is refused and nothing is written
        bad = rec.copy()
        bad["kind"][300_000] = 7
        with pytest.raises(RaftError, match="malformed") as err:
            rpl.replay(whole, bad)
        assert err.value.info["malformed"] >= 1 and err.value.info["applied"] == 0      # (its successor may count too)
        assert np.array_equal(whole.read_state(), fresh) and not whole.read_log()[0].any()
        info = rpl.replay(whole, rec)
        assert info == dict(applied=total, replicas=G * R, hardstates=G * R, truncates=0, entries=total - G * R,
                            malformed=0), info
        cuts = RP.pieces(rec, piece)
        key = rec["group"].astype(np.int64) * 8 + rec["replica"]
        assert sum(key[k * piece - 1] == key[k * piece] for k in range(1, len(cuts))) >= 2      # cuts inside runs
        tot = dict.fromkeys(RP.INFO_KEYS, 0)
        for p in cuts:
            for k, v in rpl.replay(parts, p).items():
                tot[k] += v
        assert tot["applied"] == total and tot["entries"] == total - G * R and tot["malformed"] == 0
        sw = whole.read_state()
        tw, cw = masked_logs(sw, *whole.read_log(), R)
        mt, mc = masked_logs(w, t, c, R)
        for name in ("term", "voted", "last", "phys"):
            assert np.array_equal(S.cols(sw, R, name), S.cols(w, R, name)), name
        assert np.array_equal(tw, mt) and np.array_equal(cw, mc), "the replayed logs"
        sp = parts.read_state()
        assert np.array_equal(sp, sw), "replayed in pieces"
        tp, cp = masked_logs(sp, *parts.read_log(), R)
        assert np.array_equal(tp, tw) and np.array_equal(cp, cw), "the logs replayed in pieces"
        # the volatile fields, from the model on the slices (a replay restarts the replicas it names)
        sl = on_slices(G, "lane", R)
        pick = rec[np.isin(rec["group"], sl)]
        ms, mt2, mc2 = fresh.copy(), np.zeros_like(t), np.zeros_like(c)
        minfo = RP.replay_into(whole, pick, ms, mt2, mc2)
        assert minfo["malformed"] == 0 and minfo["applied"] == len(pick)
        assert_same_state(sw[sl], ms[sl], R, "the slices against the model")
        untouched(dict(state=fresh), dict(state=ms), sl, "the model outside the slices")
