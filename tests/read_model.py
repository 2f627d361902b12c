"""Linearizable reads restated in plain Python over read_state / read_log /
sm_read arrays (include/raft_engine.h, raft_read_begin_batch,
raft_read_serve_batch): the reference of test_read_cpu.py (over the oracle and
the models of the client path and the machine) and test_gpu_read.py (against
the engine's kernels).  Nothing here calls the engine."""
from __future__ import annotations

import functools

import numpy as np

import client_model as CM
import oracle as O
import sm_model as SM
from helpers import STRESS_MIX, abi, blank_groups, fld, set_fld

ISSUED, TERM_UNCOMMITTED, NO_LEADER, UNKNOWN = (abi.READ_ISSUED, abi.READ_TERM_UNCOMMITTED, abi.READ_NO_LEADER,
                                                abi.READ_UNKNOWN)
SERVED, BEHIND, GAPPED, NO_QUORUM, DEPOSED, NONE, INVALID = (abi.READ_SERVED, abi.READ_BEHIND, abi.READ_GAPPED,
                                                             abi.READ_NO_QUORUM, abi.READ_DEPOSED, abi.READ_NONE,
                                                             abi.READ_INVALID)


def newest_leader(state, R: int, g: int) -> int:
    """The LEADER replica with the highest currentTerm, the lowest index among equals; -1 if none."""
    best, term = -1, 0
    for r in range(R):
        if fld(state, R, r, "role")[g] == abi.LEADER and (best < 0 or fld(state, R, r, "term")[g] > term):
            best, term = r, int(fld(state, R, r, "term")[g])
    return best


def begin(state, terms, groups, R: int, cap: int, W: int = 0):
    """raft_read_begin_batch over a whole engine's `state` [G, words] and
    `terms` [G, R, cap]: (tickets, return code); (None, RAFT_ERANGE) when a group
    is outside the engine (no ticket is written)."""
    groups = np.asarray(groups, dtype=np.int64)
    if len(groups) and (groups.min() < 0 or groups.max() >= state.shape[0]):
        return None, abi.RAFT_ERANGE
    tickets = np.zeros(len(groups), dtype=abi.READ_TICKET_DTYPE)
    for m, g in enumerate(groups.tolist()):
        r = newest_leader(state, R, g)
        if r < 0:
            tickets[m] = (-1, 0, -1, NO_LEADER)
            continue
        T, commit, last, phys = (int(fld(state, R, r, f)[g]) for f in ("term", "commit", "last", "phys"))
        hi = min(max(min(commit, last), 0), cap)
        if hi > 0 and W and hi - 1 < phys - W:
            st = UNKNOWN
        elif hi == 0 or int(terms[g, r, hi - 1]) != T:
            st = TERM_UNCOMMITTED
        else:
            st = ISSUED
        tickets[m] = (r, T, hi, st)
    return tickets, (abi.RAFT_EWINDOW if (tickets["status"] == UNKNOWN).any() else abi.RAFT_OK)


def serve(state, heads, regs, groups, tickets, keys, R: int, cap: int):
    """raft_read_serve_batch over `state` [G, words], `heads` [G, R] of
    abi.SM_HEAD_DTYPE and `regs` [G, R, S]: (records, return code)."""
    groups = np.asarray(groups, dtype=np.int64)
    out = np.zeros(len(groups), dtype=abi.READ_RESULT_DTYPE)
    G, S = state.shape[0], regs.shape[2]
    bad_g = bad_t = False
    for m, (g, tk, k) in enumerate(zip(groups.tolist(), tickets.tolist(), np.asarray(keys).tolist())):
        r, T, ri, st = tk
        if not 0 <= g < G:
            bad_g = True
            out[m] = (0, INVALID, 0, 0)
        elif not (0 <= r < R and 0 <= ri <= cap):
            bad_t = True
            out[m] = (0, INVALID, 0, 0)
        elif st != ISSUED:
            out[m] = (0, NONE, 0, 0)
        else:
            agree = sum(int(fld(state, R, q, "term")[g]) == T for q in range(R))
            h = heads[g, r]
            if not (fld(state, R, r, "role")[g] == abi.LEADER and fld(state, R, r, "term")[g] == T):
                out[m] = (0, DEPOSED, 0, agree)
            elif agree < R // 2 + 1:
                out[m] = (0, NO_QUORUM, 0, agree)
            elif h["applied"] < ri:
                out[m] = (0, BEHIND, h["applied"], agree)
            elif h["lost"] != 0:
                out[m] = (0, GAPPED, h["applied"], agree)
            else:
                out[m] = (regs[g, r, k & (S - 1)], SERVED, h["applied"], agree)
    return out, (abi.RAFT_ERANGE if bad_g else abi.RAFT_EINVAL if bad_t else abi.RAFT_OK)


def heads_of(G: int, R: int, applied=0, lost=0) -> np.ndarray:
    h = np.zeros((G, R), abi.SM_HEAD_DTYPE)
    h["applied"], h["lost"] = applied, lost
    return h


# ---- a crafted engine: every begin and serve situation in ten groups of five ----
CR, CG, CCAP, CS = 5, 10, 16, 8
KEY = 3                                 # the register every crafted read asks for


def crafted():
    """(state, terms, cmds, heads, regs) of 10 groups of 5 replicas.  Every
    replica holds 6 entries (terms 1 1 2 2 3 3, cmd 8 j + KEY: each lands in
    register KEY), 4 committed, currentTerm 3, and a machine that applied 4
    entries (register KEY = 8 * 3 + KEY); then
      0 no leader
      1 replica 2 leads term 3; entries 4 and 5 (term 3) committed too and applied: SERVED
      2 replica 1 leads term 3 with commit 4: log[3].term = 2 != 3, TERM_UNCOMMITTED
      3 replica 0 leads with commitIndex 0: hi == 0, TERM_UNCOMMITTED
      4 the stale leader: replica 0 still LEADER in term 3 with the old prefix (commit 4 = applied, register
        1000 + KEY); replicas 1..4 in term 4, replica 3 leads it with 7 entries committed and applied, the last
        cmd 2000 + KEY.  Begin picks replica 3; a ticket that names replica 0 serves NO_QUORUM (agree 1)
      5 as group 1, but the leader's machine stopped at 4 < 6: BEHIND
      6 as group 1, but the leader's head has lost = 1: GAPPED
      7 as group 1, but replicas 0, 3 and 4 went on to term 4 without a leader: NO_QUORUM (agree 2)
      8 two leaders of one term (replicas 1 and 4): the lower index is taken
      9 as group 1 with the leader at replica R - 1 and lastIndex 5 < commitIndex 6: hi = 5"""
    R, G, cap, S = CR, CG, CCAP, CS
    w = blank_groups(G, R)
    t = np.zeros((G, R, cap), np.int32)
    c = np.zeros((G, R, cap), np.uint32)
    t[:, :, :6] = [1, 1, 2, 2, 3, 3]
    c[:, :, :6] = 8 * np.arange(6) + KEY
    for r in range(R):
        set_fld(w, R, r, "term", 3)
        set_fld(w, R, r, "last", 6)
        set_fld(w, R, r, "phys", 6)
        set_fld(w, R, r, "commit", 4)
    heads = heads_of(G, R, applied=4)
    regs = np.zeros((G, R, S), np.uint32)
    regs[:, :, KEY] = 8 * 3 + KEY

    def lead(g, r, commit=None, applied=None):
        set_fld(w[g:g + 1], R, r, "role", abi.LEADER)
        if commit is not None:
            set_fld(w[g:g + 1], R, r, "commit", commit)
        if applied is not None:
            heads["applied"][g, r] = applied
            regs[g, r, KEY] = c[g, r, applied - 1]

    lead(1, 2, 6, 6)
    lead(2, 1)
    lead(3, 0, 0)
    lead(4, 0)
    regs[4, 0, KEY] = 1000 + KEY
    for r in range(1, R):
        set_fld(w[4:5], R, r, "term", 4)
    t[4, 3, 6], c[4, 3, 6] = 4, 2000 + KEY
    set_fld(w[4:5], R, 3, "last", 7)
    set_fld(w[4:5], R, 3, "phys", 7)
    lead(4, 3, 7, 7)
    lead(5, 2, 6)
    lead(6, 2, 6, 6)
    heads["lost"][6, 2] = 1
    lead(7, 2, 6, 6)
    for r in (0, 3, 4):
        set_fld(w[7:8], R, r, "term", 4)
    lead(8, 4, 6, 6)
    lead(8, 1, 6, 6)
    lead(9, R - 1, 6, 6)
    set_fld(w[9:10], R, R - 1, "last", 5)
    heads["applied"][9, R - 1] = 5
    regs[9, R - 1, KEY] = c[9, R - 1, 4]
    return w, t, c, heads, regs


CRAFTED_GROUPS = np.arange(CG, dtype=np.int64)
# what begin must hand out and serve must answer on the crafted engine, written out by hand
CRAFTED_TICKETS = np.array([(-1, 0, -1, NO_LEADER), (2, 3, 6, ISSUED), (1, 3, 4, TERM_UNCOMMITTED),
                            (0, 3, 0, TERM_UNCOMMITTED), (3, 4, 7, ISSUED), (2, 3, 6, ISSUED), (2, 3, 6, ISSUED),
                            (2, 3, 6, ISSUED), (1, 3, 6, ISSUED), (4, 3, 5, ISSUED)], dtype=abi.READ_TICKET_DTYPE)
CRAFTED_RECORDS = np.array([(0, INVALID, 0, 0), (43, SERVED, 6, 5), (0, NONE, 0, 0), (0, NONE, 0, 0),
                            (2003, SERVED, 7, 4), (0, BEHIND, 4, 5), (0, GAPPED, 6, 5), (0, NO_QUORUM, 0, 2),
                            (43, SERVED, 6, 5), (35, SERVED, 5, 5)], dtype=abi.READ_RESULT_DTYPE)
STALE_TICKET = np.array([(0, 3, 4, ISSUED)], dtype=abi.READ_TICKET_DTYPE)      # group 4's deposed leader
STALE_RECORD = np.array([(0, NO_QUORUM, 0, 1)], dtype=abi.READ_RESULT_DTYPE)


def small(R: int):
    """(state, terms, cmds, heads, regs) of 2 groups of R = 1 or 2 replicas,
    replica 0 leading term 2 with one entry of term 2 committed and applied
    (register KEY = 77).  R = 1: quorum 1.  R = 2: quorum 2 -- in group 1 the other
    replica is a term ahead, NO_QUORUM."""
    w = blank_groups(2, R)
    t = np.zeros((2, R, 4), np.int32)
    c = np.zeros((2, R, 4), np.uint32)
    t[:, :, 0], c[:, :, 0] = 2, 77
    for r in range(R):
        set_fld(w, R, r, "term", 2)
        set_fld(w, R, r, "last", 1)
        set_fld(w, R, r, "phys", 1)
        set_fld(w, R, r, "commit", 1)
    set_fld(w, R, 0, "role", abi.LEADER)
    if R == 2:
        set_fld(w[1:2], R, 1, "term", 3)
    regs = np.zeros((2, R, CS), np.uint32)
    regs[:, :, 77 & (CS - 1)] = 77
    return w, t, c, heads_of(2, R, applied=1), regs


def ring():
    """(state, terms, cmds) of one group of 3 in an 8-slot ring (log_cap 32):
    replica 1 leads term 2 with lastIndex 12, commitIndex 3 and physLen 12, so
    slot hi - 1 = 2 is below its window (12 - 8 = 4): UNKNOWN."""
    R, cap = 3, 32
    w = blank_groups(1, R)
    t = np.full((1, R, cap), 2, np.int32)
    c = np.zeros((1, R, cap), np.uint32)
    for r in range(R):
        set_fld(w, R, r, "term", 2)
        set_fld(w, R, r, "last", 12)
        set_fld(w, R, r, "phys", 12)
        set_fld(w, R, r, "commit", 3)
    set_fld(w, R, 1, "role", abi.LEADER)
    return w, t, c


# ---- the property: a served read reflects every write acknowledged before its begin ----
PROPERTY_KW = dict(R=5, G=203, seed=11, log_cap=300, mode=1, ae_max_entries=4, **STRESS_MIX)
PROPERTY_SLOTS = 8


def fold_value(terms, cmds, g: int, r: int, upto: int, key: int, S: int) -> int:
    """Register `key` of the last-writer fold of log[0, upto) of replica r of group g."""
    c = cmds[g, r, :upto]
    hit = np.nonzero((c & (S - 1)) == (key & (S - 1)))[0]
    return int(c[hit[-1]]) if len(hit) else 0


@functools.lru_cache(maxsize=None)
def _run(kw_items, steps, every, slots, batch_seed):
    kw = dict(kw_items)
    o = O.Oracle(abi.make_params(**kw))
    R, G, cap = kw["R"], kw["G"], kw["log_cap"]
    assert kw.get("mode", 0) == 1 and not kw.get("log_window", 0)
    rng = np.random.default_rng(batch_seed)
    mach = SM.Machine(G, R, slots)
    groups = np.arange(G, dtype=np.int64)
    all_g, all_t, all_c = np.zeros(0, np.int64), np.zeros(0, abi.TICKET_DTYPE), np.zeros(0, np.uint32)
    rounds = []
    for k in range(steps // every):
        cmds = rng.integers(1, 2 ** 32, G, dtype=np.uint32)
        ptk, prc = CM.propose(o, groups, cmds, True)
        assert prc == abi.RAFT_OK
        all_g, all_t, all_c = np.concatenate([all_g, groups]), np.concatenate([all_t, ptk]), np.concatenate([all_c, cmds])
        st = o.read_state()
        lt, lc = o.read_log()
        SM.apply(st, lt, lc, mach, R, cap)
        res, _ = CM.resolve(st, lt, lc, all_g, all_t, all_c, R, cap)
        committed = res["status"] == CM.COMMITTED
        acked = np.full(G, 0, np.int64)                             # per group: index + 1 of its highest COMMITTED ticket
        np.maximum.at(acked, all_g[committed], all_t["index"][committed].astype(np.int64) + 1)
        keys = rng.integers(0, 2 ** 32, G, dtype=np.uint32)
        heads, regs = mach.heads(), mach.reg.copy()
        tk, brc = begin(st, lt, groups, R, cap)
        # serve what begin ISSUED or held back (a NO_LEADER ticket, with its -1s, would be INVALID)
        sel = tk["replica"] >= 0
        rec = np.zeros(G, abi.READ_RESULT_DTYPE)
        rec["status"] = NONE
        rec[sel], src = serve(st, heads, regs, groups[sel], tk[sel], keys[sel], R, cap)
        rounds.append(dict(step=k * every, cmds=cmds, propose=ptk, keys=keys, tickets=tk, begin_rc=brc, sel=sel,
                           records=rec, serve_rc=src, acked=acked, state=st, heads=heads, regs=regs,
                           digest=o.digest()))
        o.step(every, counters=False)
    final = (o.read_state(), *o.read_log())
    o.close()
    return rounds, final


def property_run(steps: int = 200, every: int = 5, slots: int = PROPERTY_SLOTS, batch_seed: int = 5, **kw):
    """The oracle run for `steps` steps in rounds of `every`; each round, before
    its steps: the client model's propose for every group, the machine model's
    apply on all replicas, this model's begin for every group and serve (random keys).
    Returns (rounds, final (state, terms, cmds)); rounds[k]: step, cmds,
    propose (the tickets), keys, tickets, begin_rc, sel (the reads that were
    served: those with a leader), records, serve_rc, acked (per group: index + 1
    of its highest ticket the client model resolved COMMITTED before the begin),
    state, heads, regs, digest.  Computed once per input and shared: treat it as
    read-only."""
    return _run(tuple(sorted(kw.items())), steps, every, slots, batch_seed)


def check_property(rounds, final, R: int, slots: int, from_step: int = 100):
    """The assertions of the property on a run (the model's or the device's);
    returns the status counts of the reads from `from_step` on.
    - Value: a SERVED read's value is register `key` of the last-writer fold of
      the END-of-run log of the served replica over [0, result.applied).
    - Ordering: the read_index of every ISSUED ticket is at least index + 1 of
      every ticket of its group the client model resolved COMMITTED before the
      begin.  Returned as counts["ISSUED"]: the tickets this was asserted on."""
    _, ft, fc = final
    counts = {"reads": 0, "ISSUED": 0, "SERVED": 0, "NO_LEADER": 0, "TERM_UNCOMMITTED": 0, "NO_QUORUM": 0}
    for rd in rounds:
        tk, rec = rd["tickets"], rd["records"]
        for g in np.nonzero(rec["status"] == SERVED)[0].tolist():
            r, upto = int(tk["replica"][g]), int(rec["applied"][g])
            want = fold_value(ft, fc, g, r, upto, int(rd["keys"][g]), slots)
            assert int(rec["value"][g]) == want, (rd["step"], g, r, upto, int(rec["value"][g]), want)
            assert upto >= tk["read_index"][g], (rd["step"], g, tk[g], upto)
        issued = tk["status"] == ISSUED
        late = issued & (tk["read_index"] < rd["acked"])
        assert not late.any(), (rd["step"], np.nonzero(late)[0].tolist(), tk[late], rd["acked"][late])
        counts["ISSUED"] += int(issued.sum())
        if rd["step"] >= from_step:
            counts["reads"] += len(tk)
            counts["SERVED"] += int((rec["status"] == SERVED).sum())
            counts["NO_LEADER"] += int((tk["status"] == NO_LEADER).sum())
            counts["TERM_UNCOMMITTED"] += int((tk["status"] == TERM_UNCOMMITTED).sum())
            counts["NO_QUORUM"] += int((rec["status"] == NO_QUORUM).sum())
    return counts
