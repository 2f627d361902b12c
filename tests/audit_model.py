"""The safety audit restated in numpy over the canonical state words and the
logs (include/raft_engine.h, raft_audit_observe / raft_audit_report /
raft_audit_write): the checker of test_audit_cpu.py (crafted states and the
oracle) and test_gpu_audit.py (against the engine's kernels).  The model carries
its own ledger [G, 8 + 2 R] int32 in the exported layout; nothing here touches a
device.  observe() is vectorised over the groups (the G = 70,001 case)."""
from __future__ import annotations

import numpy as np

import snapshot_model as SM
from helpers import abi, blank_groups, fld, set_fld

TERM, VOTE, TWO, COMMIT, LEADER = (abi.AUDIT_TERM_REGRESSED, abi.AUDIT_VOTE_CHANGED, abi.AUDIT_TWO_LEADERS,
                                   abi.AUDIT_COMMIT_CHANGED, abi.AUDIT_LEADER_INCOMPLETE)
BITS = dict(zip(abi.AUDIT_KINDS, (TERM, VOTE, TWO, COMMIT, LEADER)))
# words of the exported ledger
FLAGS, FIRST, LTERM, LREP, ACOUNT, ATERM, ACMD, ASEEN = range(8)
HEAD = abi.AUDIT_HEAD


def fresh(G: int, R: int) -> np.ndarray:
    """The zero state of G ledgers."""
    L = np.zeros((G, abi.audit_words(R)), np.int32)
    L[:, LREP] = -1
    L[:, HEAD + 1::2] = -1
    return L


def zero_info() -> dict:
    return dict.fromkeys(abi.AUDIT_INFO_FIELDS, 0)


def observe(state, terms, cmds, ledger, R: int, cap: int, W: int, step: int, g0: int = 0, n=None):
    """raft_audit_observe of groups [g0, g0 + n) of a whole engine's `state`
    [G, words], logs [G, R, cap] and `ledger` [G, 8 + 2 R] (advanced in place):
    (info, return code).  W: the log_window (0: a flat log); step: the engine's
    step index.  The five steps in the header's order."""
    G = state.shape[0]
    n = G - g0 if n is None else n
    info = zero_info()
    if g0 < 0 or n < 0 or g0 + n > G:
        return info, abi.RAFT_ERANGE
    if n == 0:
        return info, abi.RAFT_OK
    st, L = state[g0:g0 + n], ledger[g0:g0 + n]
    tm, cm = terms[g0:g0 + n], np.asarray(cmds[g0:g0 + n]).astype(np.uint32).view(np.int32)
    col = lambda name: np.stack([fld(st, R, r, name) for r in range(R)], axis=1).astype(np.int64)   # [n, R]
    term, voted, role, commit, last, phys = (col(k) for k in ("term", "voted", "role", "commit", "last", "phys"))
    rr = np.arange(R)[None, :]
    rows = np.arange(n)
    bits = np.zeros(n, np.int64)
    old = L.astype(np.int64)

    # 1. term and vote
    old_t, old_v = old[:, HEAD::2], old[:, HEAD + 1::2]
    bits |= np.where((term < old_t).any(axis=1), TERM, 0)
    bits |= np.where(((term == old_t) & (old_v >= 0) & (voted != old_v)).any(axis=1), VOTE, 0)
    L[:, HEAD::2], L[:, HEAD + 1::2] = term, voted

    # 2. Election Safety
    leader = role == abi.LEADER
    two = np.zeros(n, bool)
    for a in range(R):
        for b in range(a + 1, R):
            two |= leader[:, a] & leader[:, b] & (term[:, a] == term[:, b])
    lt, lr = old[:, LTERM], old[:, LREP]
    two |= (leader & (term == lt[:, None]) & (lr[:, None] >= 0) & (rr != lr[:, None])).any(axis=1)
    bits |= np.where(two, TWO, 0)
    none = np.iinfo(np.int64).min
    key = np.where(leader, term * 8 + (7 - rr), none).max(axis=1)     # the highest term, the lowest index among equals
    newer = (key != none) & ((key >> 3) > lt)
    L[newer, LTERM], L[newer, LREP] = (key >> 3)[newer], (7 - (key & 7))[newer]

    # 3. the anchor
    C, a_term, a_cmd, a_seen = old[:, ACOUNT], old[:, ATERM], old[:, ACMD], old[:, ASEEN]
    hi = np.clip(np.minimum(commit, last), 0, cap)
    has = (C > 0)[:, None]
    i = np.clip(C - 1, 0, cap - 1)
    below = (W > 0) & ((C - 1)[:, None] < phys - W)
    at_t = np.take_along_axis(tm, i[:, None, None].repeat(R, axis=1), axis=2)[:, :, 0]
    at_c = np.take_along_axis(cm, i[:, None, None].repeat(R, axis=1), axis=2)[:, :, 0]
    same = (at_t == a_term[:, None]) & (at_c == a_cmd[:, None])
    need_a = has & (hi >= C[:, None])
    above = has & leader & (term > a_seen[:, None])
    short = above & (last < C[:, None])
    need_b = above & ~short
    bits |= np.where((need_a & ~below & ~same).any(axis=1), COMMIT, 0)
    bits |= np.where((short | (need_b & ~below & ~same)).any(axis=1), LEADER, 0)
    info["unknown"] += int((need_a & below).sum() + (need_b & below).sum())

    # 4. advance
    Cn = hi.max(axis=1)
    adv = Cn > C
    rs = np.argmax(hi == Cn[:, None], axis=1)                           # the lowest r with hi_r == C'
    i2 = np.clip(Cn - 1, 0, cap - 1)
    below_n = (W > 0) & (Cn - 1 < phys[rows, rs] - W)
    info["unknown"] += int((adv & below_n).sum())
    up = adv & ~below_n
    L[up, ACOUNT], L[up, ATERM], L[up, ACMD] = Cn[up], tm[rows, rs, i2][up], cm[rows, rs, i2][up]
    L[up, ASEEN] = term.max(axis=1)[up]

    # 5. sticky flags, the step of the first one
    was = old[:, FLAGS]
    now = was | bits
    newly = (was == 0) & (now != 0)
    L[:, FLAGS] = now
    L[newly, FIRST] = np.array(step & 0xFFFFFFFF, np.uint32).view(np.int32)
    info["newly_flagged"], info["flagged"] = int(newly.sum()), int((now != 0).sum())
    for k, b in BITS.items():
        info[k] = int(((now & ~was & b) != 0).sum())
    return info, abi.RAFT_OK


def report(ledger, g0: int = 0, n=None, max_events=None):
    """raft_audit_report of groups [g0, g0 + n): (info, events, return code).
    max_events None: room for everything."""
    G = ledger.shape[0]
    n = G - g0 if n is None else n
    info = dict.fromkeys(abi.AUDIT_REPORT_FIELDS, 0)
    none = np.zeros(0, abi.AUDIT_EVENT_DTYPE)
    if g0 < 0 or n < 0 or g0 + n > G:
        return info, none, abi.RAFT_ERANGE
    if max_events is not None and max_events < 0:
        return info, none, abi.RAFT_EINVAL
    hit = np.nonzero(ledger[g0:g0 + n, FLAGS])[0]
    room = len(hit) if max_events is None else min(int(max_events), len(hit))
    take = hit[:room]
    ev = np.zeros(room, abi.AUDIT_EVENT_DTYPE)
    ev["group"], ev["flags"], ev["first_step"] = g0 + take, ledger[g0 + take, FLAGS], ledger[g0 + take, FIRST]
    info["delivered"], info["pending"], info["flagged"] = room, len(hit) - room, len(hit)
    return info, ev, abi.RAFT_OK


def valid_ledger(ledger, R: int, cap: int) -> bool:
    """raft_audit_write's rule: known flag bits, lead_replica in -1..R-1, anchor_count in 0..log_cap."""
    a = np.asarray(ledger, dtype=np.int64).reshape(-1, abi.audit_words(R))
    return bool((((a[:, FLAGS] & ~abi.AUDIT_ALL) == 0) & (a[:, LREP] >= -1) & (a[:, LREP] < R) & (a[:, ACOUNT] >= 0)
                 & (a[:, ACOUNT] <= cap)).all())


class Host(SM.Host):
    """snapshot_model's Host (the oracle under RaftEngine's method names, with
    restart, install and heal) with audits: each ledger of `ledgers` is an
    audit of its own, observed when the caller says."""

    def __init__(self, slots: int, **kw):
        super().__init__(slots, **kw)
        self.ledgers = {}

    def observe(self, name: str = "audit", g0: int = 0, n=None) -> dict:
        L = self.ledgers.setdefault(name, fresh(self.G, self.R))
        info, rc = observe(self.o.read_state(), *self.o.read_log(), L, self.R, self.cap, self.W, self.step_index, g0, n)
        assert rc == abi.RAFT_OK
        return info


# ---- crafted groups: one per rule and per non-case, R = 3, log_cap 16, each in
# two phases (a state, an observe at step CRAFTED_STEPS[0]; a second state, an
# observe at CRAFTED_STEPS[1]) from the zero ledger.  Expected: the flags after
# each phase, written out by hand.
CR, CCAP = 3, 16
CRAFTED_STEPS = (5, 9)
F_, L_ = abi.FOLLOWER, abi.LEADER


def _rep(term=0, voted=-1, role=F_, commit=0, log=(), last=None, phys=None):
    return dict(term=term, voted=voted, role=role, commit=commit, log=list(log), last=len(log) if last is None else last,
                phys=phys)


E2 = [(1, 10), (1, 11)]                                                 # two entries of term 1
E4 = [(1, 10), (1, 11), (1, 12), (1, 13)]
_all3 = lambda **kw: [_rep(**kw) for _ in range(3)]

# name: (phase 0, phase 1, flags after phase 0, flags after phase 1)
CRAFTED = {
    # two LEADERs of term 3 at one observe
    "two_now": ([_rep(3, 0, L_), _rep(3, 1, L_), _rep(3, 0)],) * 2 + (TWO, TWO),
    # replica 0 leads term 3 at the first observe, replica 1 leads term 3 at the second
    # (replica 1 had not voted when first seen: its vote for itself is no change)
    "two_across": ([_rep(3, 0, L_), _rep(3, -1), _rep(3, 0)], [_rep(3, 0), _rep(3, 1, L_), _rep(3, 0)], 0, TWO),
    "term_lowered": (_all3(term=4, voted=1), [_rep(4, 1), _rep(4, 1), _rep(2, -1)], 0, TERM),
    "vote_changed": (_all3(term=4, voted=0), [_rep(4, 0), _rep(4, 2), _rep(4, 0)], 0, VOTE),
    # a vote reset by a higher term is no violation
    "vote_new_term": (_all3(term=4, voted=0), [_rep(4, 0), _rep(5, 2), _rep(4, 0)], 0, 0),
    # the anchor is (2, (1, 11)); replica 1 then holds (2, 99) at index 1 inside its committed prefix
    "commit_rewritten": ([_rep(1, 0, L_, 2, E2), _rep(1, 0, F_, 2, E2), _rep(1, 0, F_, 2, E2)],
                         [_rep(1, 0, L_, 2, E2), _rep(1, 0, F_, 2, [(1, 10), (2, 99)]), _rep(1, 0, F_, 2, E2)],
                         0, COMMIT),
    # a leader of term 2 > anchor_seen_term 1 whose log ends below the anchor
    "leader_short": ([_rep(1, 0, L_, 2, E2), _rep(1, 0, F_, 2, E2), _rep(1, 0, F_, 2, E2)],
                     [_rep(2, 2, F_, 2, E2), _rep(2, 2, F_, 2, E2), _rep(2, 2, L_, 0, E2[:1])], 0, LEADER),
    # ... and one that holds another entry there (not committed on it: no COMMIT_CHANGED)
    "leader_differs": ([_rep(1, 0, L_, 2, E2), _rep(1, 0, F_, 2, E2), _rep(1, 0, F_, 2, E2)],
                       [_rep(2, 2, F_, 2, E2), _rep(2, 2, F_, 2, E2), _rep(2, 2, L_, 0, [(1, 10), (1, 77)])],
                       0, LEADER),
    # ---- the non-cases
    # a deposed leader keeps its role at a lower term
    "deposed_lower": ([_rep(2, 0, L_), _rep(2, 0), _rep(2, 0)], [_rep(2, 0, L_), _rep(3, 1, L_), _rep(3, 1)], 0, 0),
    # Figure 8: replica 2, isolated, is still LEADER of term 2 <= anchor_seen_term 3 and lacks the anchor
    "figure8": ([_rep(3, 0, L_, 2, E2), _rep(3, 0, F_, 2, E2), _rep(2, 2, L_, 0, E2[:1])],) * 2 + (0, 0),
    # a persistent restart puts commitIndex back to 0
    "commit_zero": (_all3(term=1, voted=0, commit=2, log=E2),
                    [_rep(1, 0, F_, 2, E2), _rep(1, 0, F_, 0, E2), _rep(1, 0, F_, 2, E2)], 0, 0),
    # C advances by several entries between two observes
    "advance_many": (_all3(term=1, voted=0, commit=1, log=E4), _all3(term=1, voted=0, commit=4, log=E4), 0, 0),
    # first_step is the first violation's: two leaders at the first observe, a term lowered at the second
    "first_kept": ([_rep(3, 0, L_), _rep(3, 1, L_), _rep(3, 0)], [_rep(3, 0, L_), _rep(3, 1, L_), _rep(1, 0)],
                   TWO, TWO | TERM),
}
CRAFTED_NAMES = list(CRAFTED)
# selected ledger words after phase 1: name -> {word: value}
CRAFTED_WORDS = {
    "two_now": {FIRST: 5, LTERM: 3, LREP: 0},
    "two_across": {FIRST: 9, LTERM: 3, LREP: 0},
    "term_lowered": {FIRST: 9, HEAD + 4: 2, HEAD + 5: -1},
    "vote_new_term": {HEAD + 2: 5, HEAD + 3: 2},
    "commit_rewritten": {FIRST: 9, ACOUNT: 2, ATERM: 1, ACMD: 11, ASEEN: 1},
    "leader_short": {FIRST: 9, LTERM: 2, LREP: 2, ACOUNT: 2},
    "deposed_lower": {FIRST: 0, LTERM: 3, LREP: 1},
    "figure8": {ACOUNT: 2, ASEEN: 3, LTERM: 3, LREP: 0},
    "commit_zero": {ACOUNT: 2, ATERM: 1, ACMD: 11},
    "advance_many": {ACOUNT: 4, ATERM: 1, ACMD: 13, ASEEN: 1},
    "first_kept": {FIRST: 5},
}


def build(groups, R: int, cap: int):
    """(state, terms, cmds) of a list of groups, each a list of R _rep dicts."""
    n = len(groups)
    w = blank_groups(n, R)
    terms, cmds = np.zeros((n, R, cap), np.int32), np.zeros((n, R, cap), np.uint32)
    for g, reps in enumerate(groups):
        one = w[g:g + 1]
        for r, x in enumerate(reps):
            for k in ("term", "voted", "role", "commit", "last"):
                set_fld(one, R, r, k, x[k])
            set_fld(one, R, r, "phys", x["last"] if x["phys"] is None else x["phys"])
            for j, (t, c) in enumerate(x["log"]):
                terms[g, r, j], cmds[g, r, j] = t, c
    return w, terms, cmds


def crafted_phase(k: int):
    """(state, terms, cmds) of phase k of every crafted group."""
    return build([CRAFTED[name][k] for name in CRAFTED_NAMES], CR, CCAP)


def crafted_flags(k: int) -> np.ndarray:
    return np.array([CRAFTED[name][2 + k] for name in CRAFTED_NAMES], np.int32)


# ---- the same on a 16-slot ring (log_window 16, log_cap 128): slots below a window are not read
RING_W, RING_CAP = 16, 128
_run = lambda n, t=1: [(t, 100 + j) for j in range(n)]


def _ring_rep(term, role, commit, n):
    """A replica whose log has n entries (term 1, cmd 100 + j); only its window's slots matter."""
    return _rep(term, 0, role, commit, _run(n))


RING = {
    # the anchor (10, (1, 109)) is recorded; replica 0 then moves on to 40 entries as LEADER of term 2: slot 9 is
    # below its window [24, 40), so both of its checks are skipped (unknown 2); replicas 1 and 2 still hold it; the
    # new anchor's slot 39 is inside the window
    "below_window": (_all3(term=1, voted=0, commit=10, log=_run(10)),
                     [_ring_rep(2, L_, 40, 40), _ring_rep(1, F_, 10, 10), _ring_rep(1, F_, 10, 10)]),
    # commitIndex 40 of 80 entries: slot 39 is below the window [64, 80), the anchor cannot be recorded
    "advance_below": ([_rep(1, 0, F_, 40, _run(80))] * 3,) * 2,
}
RING_NAMES = list(RING)
RING_UNKNOWN = (1, 3)                                                   # per phase, over both groups
RING_WORDS = {"below_window": {FLAGS: 0, ACOUNT: 40, ATERM: 1, ACMD: 139, ASEEN: 2},
              "advance_below": {FLAGS: 0, ACOUNT: 0}}


def ring_phase(k: int):
    return build([RING[name][k] for name in RING_NAMES], CR, RING_CAP)


# ---- groups built in numpy, never stepped (the G = 70,001 case): every 7th group raises one of the five flags in
# rotation at the second observe
def bulk(G: int, R: int = 3, cap: int = 16):
    """((state, terms, cmds) of phase 0, of phase 1, the flags expected after phase 1).  Every group: replica 0
    leads term 2, two committed entries everywhere.  Group g with g % 7 == 0 breaks rule (g // 7) % 5 in phase 1."""
    base = [_rep(2, 0, L_, 2, E2), _rep(2, 0, F_, 2, E2), _rep(2, 0, F_, 2, E2)]
    bad = [
        [_rep(2, 0, L_, 2, E2), _rep(1, 0, F_, 2, E2), _rep(2, 0, F_, 2, E2)],                       # TERM
        [_rep(2, 0, L_, 2, E2), _rep(2, 1, F_, 2, E2), _rep(2, 0, F_, 2, E2)],                       # VOTE
        [_rep(2, 0, F_, 2, E2), _rep(2, 0, L_, 2, E2), _rep(2, 0, F_, 2, E2)],                       # TWO (across)
        [_rep(2, 0, L_, 2, E2), _rep(2, 0, F_, 2, E2), _rep(2, 0, F_, 2, [(1, 10), (2, 5)])],        # COMMIT
        [_rep(3, 1, F_, 2, E2), _rep(3, 1, L_, 0, E2[:1]), _rep(3, 1, F_, 2, E2)],                   # LEADER
    ]
    kinds = (TERM, VOTE, TWO, COMMIT, LEADER)
    one = build([base] + bad, R, cap)
    pick = np.zeros(G, np.int64)
    hit = np.arange(0, G, 7)
    pick[hit] = 1 + (hit // 7) % 5
    want = np.zeros(G, np.int32)
    want[hit] = np.array(kinds, np.int32)[(hit // 7) % 5]
    p0 = tuple(a[np.zeros(G, np.int64)] for a in one)
    p1 = tuple(a[pick] for a in one)
    return p0, p1, want
