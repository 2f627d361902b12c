"""Leader no-op entries on the CPU: the model (noop_model.py) on crafted states
and over the oracle -- what test_gpu_noop.py holds the engine's kernel to --
and the premise of the feature on the oracle alone.  No device is touched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import client_model as CM
import noop_model as NM
import oracle as O
import sm_model as M
from helpers import abi, blank_groups, fld, log_matching_flags, set_fld, set_session

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = pytest.mark.parametrize("textbook", [False, True], ids=["reference", "textbook"])


def crafted_oracle(textbook: bool, ring: bool = False):
    w, t, c = NM.crafted_ring(textbook) if ring else NM.crafted()
    kw = dict(R=NM.CR, G=len(w), log_cap=t.shape[2], **(dict(mode=abi.MODE_TEXTBOOK) if textbook else {}),
              **(dict(log_window=NM.RING_W) if ring else {}))
    o = O.Oracle(abi.make_params(**kw))
    o.write_state(w)
    o.write_log(t, c)
    assert np.array_equal(o.read_state(), w)
    return o, w, t, c


@MODES
def test_every_record_kind_on_crafted_states(textbook):
    """One group per record kind: the tickets, ticket_cmds and info are the ones
    written out by hand, and the oracle ends where raft_append_command_batch
    with (group, L, cmd) on the appended groups leaves a second oracle."""
    o, w, t, c = crafted_oracle(textbook)
    want_tk, want_c, want_info = NM.crafted_want(textbook)
    info, tk, tc, rc = NM.append_noops(o, 0, len(w), NM.NOOP, textbook)
    assert rc == abi.RAFT_OK and info == want_info
    for name, a, b in zip(NM.CRAFTED_NAMES, tk.tolist(), want_tk.tolist()):
        assert a == b, (name, a, b)
    assert tc.tolist() == want_c.tolist()
    assert set(tk["status"].tolist()) == {NM.ACCEPTED, NM.NO_LEADER, NM.LOG_FULL, NM.CURRENT} | \
        (set() if textbook else {NM.GHOSTED})
    o2, *_ = crafted_oracle(textbook)
    for g in np.nonzero((tk["status"] == NM.ACCEPTED) | (tk["status"] == NM.GHOSTED))[0].tolist():
        o2.append_command(g, int(tk["replica"][g]), NM.NOOP)
    assert np.array_equal(o.read_state(), o2.read_state()) and o.digest() == o2.digest()
    # the tickets go to resolve unchanged: NONE where nothing was stored, PENDING where the leader holds the entry
    # (GHOSTED: the slot the ticket names shows a stale entry, LOST, as a ghosted proposal's)
    rec, rrc = CM.resolve(o.read_state(), *o.read_log(), np.arange(len(w)), tk, tc, NM.CR, NM.CCAP)
    want = {NM.NO_LEADER: CM.NONE, NM.LOG_FULL: CM.NONE, NM.ACCEPTED: CM.PENDING, NM.CURRENT: CM.PENDING,
            NM.GHOSTED: CM.LOST}
    assert rrc == abi.RAFT_OK and rec["status"].tolist() == [want[s] for s in tk["status"].tolist()]
    # a part of the range: the records of groups [2, 5) alone
    o3, *_ = crafted_oracle(textbook)
    info3, tk3, tc3, _ = NM.append_noops(o3, 2, 3, NM.NOOP, textbook)
    assert tk3.tolist() == want_tk[2:5].tolist() and tc3.tolist() == want_c[2:5].tolist()
    assert info3 == dict(appended=2, current=1, no_leader=0, log_full=0, ghosted=0)
    for x in (o, o2, o3):
        x.close()


@MODES
def test_a_second_call_appends_nothing(textbook):
    o, w, *_ = crafted_oracle(textbook)
    _, tk, _, _ = NM.append_noops(o, 0, len(w), NM.NOOP, textbook)
    before, dg = o.read_state(), o.digest()
    info, tk2, tc2, rc = NM.append_noops(o, 0, len(w), NM.NOOP + 1, textbook)
    kept = (tk["status"] == NM.NO_LEADER) | (tk["status"] == NM.LOG_FULL)
    assert info["appended"] == 0 and info["current"] == int((~kept).sum()) and rc == abi.RAFT_OK
    assert (tk2["status"][~kept] == NM.CURRENT).all() and np.array_equal(tk2[kept], tk[kept])
    assert np.array_equal(o.read_state(), before) and o.digest() == dg
    # a CURRENT ticket names the tail entry: where the first call stored its entry, that entry
    stored = tk["status"] == NM.ACCEPTED
    assert np.array_equal(tk2["index"][stored], tk["index"][stored]) and (tc2[stored] == NM.NOOP).all()
    o.close()


@MODES
def test_a_wrapped_window_and_an_add_below_it(textbook):
    o, w, *_ = crafted_oracle(textbook, ring=True)
    want_tk, want_c, want_info, want_rc = NM.crafted_ring_want(textbook)
    info, tk, tc, rc = NM.append_noops(o, 0, len(w), NM.NOOP, textbook, NM.RING_W)
    assert (info, tk.tolist(), tc.tolist(), rc) == (want_info, want_tk.tolist(), want_c.tolist(), want_rc)
    o.close()


def test_abi_symbols_and_record_sizes():
    lib = abi.load_library()
    assert C.sizeof(abi.raft_noop_info) == 64 == abi.NOOP_INFO_DTYPE.itemsize
    hdr = open(os.path.join(ROOT, "include", "raft_engine.h")).read()
    assert int(re.search(r"#define RAFT_PROPOSE_CURRENT\s+(\d+)", hdr).group(1)) == abi.PROPOSE_CURRENT == 4
    m = re.search(r"typedef struct raft_noop_info \{(.*?)\} raft_noop_info;", hdr, re.S)
    assert re.findall(r"int64_t\s+(\w+)", m.group(1)) == [n for n, _ in abi.raft_noop_info._fields_]
    assert [n for n, _ in abi.raft_noop_info._fields_][:-1] == list(abi.NOOP_INFO_FIELDS) == list(abi.NOOP_INFO_DTYPE.names[:-1])
    for name in ("raft_engine_append_noops", "raft_engine_append_noops_dev", "raft_engine_sm_set_noop"):
        assert name in abi.EXPORTED_SYMBOLS and getattr(lib, name).restype is C.c_int
    assert "This engine has no no-op" not in hdr and lib.raft_abi_version() == 2


def test_einval_without_a_device():
    """A null engine is refused by every form before anything else."""
    lib = abi.load_library()
    info = abi.raft_noop_info()
    buf = np.zeros(64, np.uint8).ctypes.data
    for fn in (lib.raft_engine_append_noops, lib.raft_engine_append_noops_dev):
        assert fn(None, 0, 4, 7, buf, buf, C.byref(info)) == abi.RAFT_EINVAL and b"null engine" in lib.raft_last_error()
    assert lib.raft_engine_sm_set_noop(None, 1, 7) == abi.RAFT_EINVAL and b"null engine" in lib.raft_last_error()


# ---- the premise, on the oracle alone ----
PREMISE_STEPS = 2          # steps after the no-op until a majority has commitIndex 3 (from the oracle run made here)


def test_entries_of_earlier_terms_wait_for_an_entry_of_the_new_term():
    """Textbook mode, R = 5, no drops, no commands: a term-3 leader and its
    followers hold the same two entries of terms 1 and 2, uncommitted, the
    sessions caught up.  The commit rule's current-term guard keeps commitIndex
    at 0 on every replica through 30 steps; after the no-op a majority of every
    group has commitIndex 3 within PREMISE_STEPS steps."""
    R, G, cap, L = 5, 16, 16, 1
    w = blank_groups(G, R)
    t = np.zeros((G, R, cap), np.int32)
    c = np.zeros((G, R, cap), np.uint32)
    t[:, :, 0], t[:, :, 1] = 1, 2
    c[:, :, 0], c[:, :, 1] = 71, 72
    for r in range(R):
        set_fld(w, R, r, "term", 3)
        set_fld(w, R, r, "voted", L + 1)
        set_fld(w, R, r, "last", 2)
        set_fld(w, R, r, "phys", 2)
        set_fld(w, R, r, "flags", abi.FL_ARMED)
        set_fld(w, R, r, "election_ms", 20000 + r)
    set_fld(w, R, L, "role", abi.LEADER)
    set_fld(w, R, L, "flags", abi.FL_HB_ACTIVE)
    set_fld(w, R, L, "election_ms", 0)
    set_session(w, R, L, [3] * R, [2] * R)                          # nextIndex = lastIndex + 1, matchIndex = lastIndex
    o = O.Oracle(abi.make_params(R=R, G=G, log_cap=cap, seed=5, mode=abi.MODE_TEXTBOOK, cmd_ppm=0))
    o.write_state(w)
    o.write_log(t, c)
    commits = lambda: np.stack([fld(o.read_state(), R, r, "commit") for r in range(R)], -1)
    for _ in range(30):
        rows = o.step(1)
        assert (commits() == 0).all() and rows[0, abi.C_INDEX["leaders"]] == G
    assert (fld(o.read_state(), R, L, "term") == 3).all()          # the same leader, the same term: nothing moved
    info, tk, _, _ = NM.append_noops(o, 0, G, NM.NOOP, True)
    assert info["appended"] == G and tk.tolist() == [(L, 2, 3, NM.ACCEPTED)] * G
    o.step(PREMISE_STEPS)
    assert ((commits() == 3).sum(axis=1) >= R // 2 + 1).all(), commits()
    o.close()


# ---- the state machine passes over the entry ----
def test_the_machine_skips_the_entry_in_its_registers_only():
    """sm_apply with the skip: applied and hash are the fold of the whole log,
    the registers the fold of the log without the no-op entries."""
    rng = np.random.default_rng(3)
    R, G, cap, S = 3, 6, 24, 4
    w = blank_groups(G, R)
    t = np.sort(rng.integers(1, 5, (G, R, cap)), axis=2).astype(np.int32)
    c = rng.integers(1, 2 ** 32, (G, R, cap), dtype=np.uint32)
    noop = 0xABCD0002                                               # lands in slot 2
    c[rng.random((G, R, cap)) < 0.3] = noop
    c[0, 0, :] = noop                                               # a log of nothing else
    c[1, 1, cap - 1] = noop                                         # the last applied entry is one
    n = rng.integers(0, cap + 1, (G, R))
    n[0, 0] = n[1, 1] = cap
    for r in range(R):
        set_fld(w, R, r, "last", n[:, r])
        set_fld(w, R, r, "phys", n[:, r])
        set_fld(w, R, r, "commit", n[:, r])
    skip, plain, filtered = (M.Machine(G, R, S) for _ in range(3))
    info = NM.sm_apply(w, t, c, skip, R, cap, noop=noop)
    assert info == M.apply(w, t, c, plain, R, cap) and info["applied"] == int(n.sum())
    assert np.array_equal(skip.heads(), plain.heads())
    # the registers: sm_model on logs with the no-ops taken out
    ft, fc, fw = np.zeros_like(t), np.zeros_like(c), w.copy()
    for g in range(G):
        for r in range(R):
            keep = np.nonzero(c[g, r, :n[g, r]] != noop)[0]
            ft[g, r, :len(keep)], fc[g, r, :len(keep)] = t[g, r, keep], c[g, r, keep]
            for f in ("last", "phys", "commit"):
                fw[g, r * abi.NUM_FIELDS + abi.F_INDEX[f]] = len(keep)
    M.apply(fw, ft, fc, filtered, R, cap)
    assert np.array_equal(skip.reg, filtered.reg) and not np.array_equal(skip.reg, plain.reg)
    assert (skip.reg[0, 0] == 0).all() and (skip.reg != noop).all() and (plain.reg == noop).any()
    # in two parts, the cursor between them: the same machine
    half = M.Machine(G, R, S)
    wh = w.copy()
    for r in range(R):
        set_fld(wh, R, r, "commit", n[:, r] // 2)
    NM.sm_apply(wh, t, c, half, R, cap, noop=noop)
    NM.sm_apply(w, t, c, half, R, cap, noop=noop)
    assert np.array_equal(half.heads(), skip.heads()) and np.array_equal(half.reg, skip.reg)
    # disabled is sm_model itself
    off = M.Machine(G, R, S)
    NM.sm_apply(w, t, c, off, R, cap)
    assert np.array_equal(off.reg, plain.reg) and np.array_equal(off.heads(), plain.heads())


# ---- over the oracle ----
def test_the_parity_scenario_is_not_vacuous():
    """Over the parity cases the two calls meet every status but LOG_FULL, the
    first call appends and the settle steps commit some of the entries."""
    seen, tot = set(), dict.fromkeys(abi.NOOP_INFO_FIELDS, 0)
    committed = 0
    for R, G, v in NM.PARITY_CASES:
        points, _ = NM.host_parity_run(R, G, v)
        by = {p["what"].split()[-1]: p for p in points}
        for k in ("noops", "again"):
            seen |= set(by[k]["tickets"]["status"].tolist())
            for f in tot:
                tot[f] += by[k]["info"][f]
            assert sum(by[k]["info"][f] for f in ("appended", "current", "no_leader", "log_full")) == max(G - 5, 0)
        first = by["noops"]["tickets"]["status"]
        committed += int((by["resolve"]["states"]["status"][(first == NM.ACCEPTED)] == CM.COMMITTED).sum())
    assert seen == {NM.ACCEPTED, NM.GHOSTED, NM.NO_LEADER, NM.CURRENT}, seen
    assert tot["appended"] > 50 and tot["current"] > 50 and tot["ghosted"] > 0 and committed > 0, (tot, committed)


def test_idle_groups_serve_reads_after_the_entry():
    """cmd_ppm = 0: every read begins TERM_UNCOMMITTED; one no-op per group and
    the steps it takes to commit, and every ticket is COMMITTED and every read
    ISSUED."""
    r = NM.host_idle_reads()
    G = NM.LIVE_KW["G"]
    assert (r["before"]["status"] == abi.READ_TERM_UNCOMMITTED).all() and (r["before"]["read_index"] == 0).all()
    assert r["info"] == dict(appended=G, current=0, no_leader=0, log_full=0, ghosted=0)
    assert (r["tickets"]["status"] == NM.ACCEPTED).all() and (r["tickets"]["index"] == 0).all()
    assert 1 <= r["settle"] <= 3
    assert (r["resolved"]["status"] == CM.COMMITTED).all()
    assert (r["after"]["status"] == abi.READ_ISSUED).all() and (r["after"]["read_index"] == 1).all()


def test_without_the_entry_an_idle_group_never_serves():
    """The same engine left alone for 60 more steps: still TERM_UNCOMMITTED."""
    h = NM.Host(**NM.LIVE_KW)
    NM.step_until(h, NM.all_led(h))
    h.step(60)
    tk = h.begin_reads(np.arange(h.G))
    h.close()
    assert (tk["status"] == abi.READ_TERM_UNCOMMITTED).all()


def test_stalled_tickets_are_released():
    """An evacuate and a proposal between two steps: the groups replica 0 led
    change leaders, their tickets are still PENDING 30 steps into the new term,
    and none is once the new leaders have their no-op.  No group ever has two
    leaders of one term, and Log Matching holds."""
    s = NM.host_stalled_tickets()
    assert s["evacuate"]["sent"] == len(s["led0"]) > 0
    assert s["stalled"] and set(s["stalled"]) <= set(s["led0"])
    assert s["info"]["appended"] >= len(s["stalled"]) and 1 <= s["settle"] <= 3
    assert (s["final"]["status"][s["stalled"]] != CM.PENDING).all()
    others = np.setdiff1d(np.arange(NM.LIVE_KW["G"]), s["led0"])
    assert (s["later"]["status"][others] == CM.COMMITTED).all()      # an undisturbed leader commits its own term's entry
    assert s["dual"] == 0 and s["matching"] == 0
