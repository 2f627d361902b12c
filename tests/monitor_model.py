"""The liveness monitor restated in numpy over the canonical state words
(include/raft_engine.h, raft_monitor_observe / raft_monitor_report /
raft_monitor_write / raft_monitor_set_availability): the checker of
test_monitor_cpu.py (crafted states and the oracle) and test_gpu_monitor.py
(against the engine's kernels).  The model carries its own ledger [G, 16] int32
in the exported layout and its own availability totals; nothing here touches a
device.  observe() is vectorised over the groups (the G = 70,001 case)."""
from __future__ import annotations

import numpy as np

from helpers import abi, blank_groups, fld, set_fld

LL, ST, LAG, CH = abi.MONITOR_LEADERLESS, abi.MONITOR_COMMIT_STALLED, abi.MONITOR_LAGGING, abi.MONITOR_CHURNING
BITS = dict(zip(abi.MONITOR_KINDS, (LL, ST, LAG, CH)))
# words of the exported ledger
(NOW, EVER, FIRST, LEADER, DOWN_SINCE, OUTAGES, DOWN_TOTAL, LONGEST, STALL_SINCE, STALL_MARK, WIN_START, WIN_TERM,
 LAG_MASK, MAX_LAG, RSV0, RSV1) = range(abi.MONITOR_WORDS)
I32_MAX = 2 ** 31 - 1


def fresh(G: int) -> np.ndarray:
    """The zero state of G ledgers."""
    L = np.zeros((G, abi.MONITOR_WORDS), np.int32)
    L[:, [LEADER, DOWN_SINCE, STALL_SINCE, WIN_START]] = -1
    return L


def zero_avail() -> dict:
    return {"hist": np.zeros(abi.MONITOR_HIST, np.int64), "outages": 0, "down_steps": 0}


def same_avail(a: dict, b: dict) -> bool:
    return np.array_equal(a["hist"], b["hist"]) and (a["outages"], a["down_steps"]) == (b["outages"], b["down_steps"])


def config(**kw) -> dict:
    """A raft_monitor_config as a dict; RaftEngine.monitor's defaults."""
    c = dict(leaderless_steps=0, stalled_steps=abi.MONITOR_STALLED_STEPS, lag_entries=0, churn_terms=0, churn_steps=1)
    assert set(kw) <= set(c), kw
    c.update(kw)
    return c


def valid_config(c: dict, reserved=(0, 0, 0)) -> bool:
    """raft_monitor_create's rule."""
    return (all(c[k] >= 0 for k in abi.MONITOR_CONFIG_FIELDS) and not (c["churn_terms"] > 0 and c["churn_steps"] < 1)
            and not any(reserved))


def zero_info() -> dict:
    return dict.fromkeys(abi.MONITOR_INFO_FIELDS, 0)


def step32(step: int) -> int:
    """The low 32 bits of a step index as the int32 the ledger stores."""
    return int(np.array(step & 0xFFFFFFFF, np.uint32).view(np.int32))


def age(s: int, x):
    """max(0, (int32)(s - x)), the subtraction taken mod 2^32; x an int64 array of int32 values."""
    d = (s - np.asarray(x, np.int64)) & 0xFFFFFFFF
    d = np.where(d >= 2 ** 31, d - 2 ** 32, d)
    return np.maximum(d, 0)


def observe(state, ledger, avail, cfg, R: int, cap: int, step: int, g0: int = 0, n=None):
    """raft_monitor_observe of groups [g0, g0 + n) of a whole engine's `state`
    [G, words] and `ledger` [G, 16] (advanced in place, as `avail` is):
    (info, return code).  step: the engine's step index.  The five rules in the
    header's order."""
    G = state.shape[0]
    n = G - g0 if n is None else n
    info = zero_info()
    if g0 < 0 or n < 0 or g0 + n > G:
        return info, abi.RAFT_ERANGE
    if n == 0:
        return info, abi.RAFT_OK
    st, Lg = state[g0:g0 + n], ledger[g0:g0 + n]
    col = lambda name: np.stack([fld(st, R, r, name) for r in range(R)], axis=1).astype(np.int64)   # [n, R]
    term, role, commit, last = (col(k) for k in ("term", "role", "commit", "last"))
    rr = np.arange(R)[None, :]
    rows = np.arange(n)
    old = Lg.astype(np.int64)
    s = step32(step)
    now = np.zeros(n, np.int64)

    # the newest leader: the highest term, the lowest index among equals
    is_leader = role == abi.LEADER
    none = np.iinfo(np.int64).min
    key = np.where(is_leader, term * 8 + (7 - rr), none).max(axis=1)
    Ld = np.where(key == none, -1, 7 - (key & 7))
    has = Ld >= 0
    Lc = np.maximum(Ld, 0)
    hi = np.clip(np.minimum(commit, last), 0, cap)
    last_L, hi_L = last[rows, Lc], hi[rows, Lc]
    T = term.max(axis=1)

    # 1. outage
    ds = old[:, DOWN_SINCE].copy()
    start = ~has & (ds == -1)
    ds[start] = s
    now |= np.where(~has & (age(s, ds) >= cfg["leaderless_steps"]), LL, 0)
    ended = has & (old[:, DOWN_SINCE] != -1)
    length = np.maximum(1, age(s, old[:, DOWN_SINCE]))
    ds[ended] = -1
    Lg[:, DOWN_SINCE] = ds
    Lg[:, OUTAGES] = np.where(ended, np.minimum(old[:, OUTAGES] + 1, I32_MAX), old[:, OUTAGES])
    Lg[:, DOWN_TOTAL] = np.where(ended, np.minimum(old[:, DOWN_TOTAL] + length, I32_MAX), old[:, DOWN_TOTAL])
    Lg[:, LONGEST] = np.where(ended, np.maximum(old[:, LONGEST], length), old[:, LONGEST])
    for ln in length[ended].tolist():
        avail["hist"][int(ln).bit_length() - 1] += 1
    avail["outages"] += int(ended.sum())
    avail["down_steps"] += int(length[ended].sum())

    # 2. stalled commit
    backlog = has & (last_L > hi_L)
    ss, mark = old[:, STALL_SINCE].copy(), old[:, STALL_MARK].copy()
    moved = backlog & ((ss == -1) | (hi_L > mark))
    ss[moved], mark[moved] = s, hi_L[moved]
    ss[~backlog], mark[~backlog] = -1, 0
    now |= np.where(backlog & (age(s, ss) >= cfg["stalled_steps"]), ST, 0)
    Lg[:, STALL_SINCE], Lg[:, STALL_MARK] = ss, mark

    # 3. lag behind the newest leader
    on = has & (cfg["lag_entries"] > 0)
    lag = last_L[:, None] - last
    other = on[:, None] & (rr != Ld[:, None])
    mask = ((other & (lag >= cfg["lag_entries"])) * (1 << rr)).sum(axis=1)
    Lg[:, LAG_MASK] = mask
    Lg[:, MAX_LAG] = np.where(other, np.clip(lag, 0, I32_MAX), 0).max(axis=1)
    now |= np.where(mask != 0, LAG, 0)

    # 4. churn
    if cfg["churn_terms"] > 0:
        ws, wt = old[:, WIN_START].copy(), old[:, WIN_TERM].copy()
        new = ws == -1
        ws[new], wt[new] = s, T[new]
        now |= np.where(T - wt >= cfg["churn_terms"], CH, 0)
        roll = age(s, ws) >= cfg["churn_steps"]
        ws[roll], wt[roll] = s, T[roll]
        Lg[:, WIN_START], Lg[:, WIN_TERM] = ws, wt

    # 5. bookkeeping
    was, ever_was = old[:, NOW], old[:, EVER]
    ever = ever_was | now
    Lg[:, NOW], Lg[:, EVER], Lg[:, LEADER] = now, ever, Ld
    Lg[(ever_was == 0) & (ever != 0), FIRST] = s
    info["flagged"] = int((now != 0).sum())
    info["newly_flagged"] = int(((was == 0) & (now != 0)).sum())
    info["cleared"] = int(((was != 0) & (now == 0)).sum())
    for k, b in BITS.items():
        info[k] = int(((now & b) != 0).sum())
    info["down"] = int((ds != -1).sum())
    info["outages_ended"], info["down_steps_ended"] = int(ended.sum()), int(length[ended].sum())
    return info, abi.RAFT_OK


def report(ledger, g0: int = 0, n=None, max_events=None, ever: bool = False, kinds: int = abi.MONITOR_ALL):
    """raft_monitor_report of groups [g0, g0 + n): (info, events, return code).
    max_events None: room for everything."""
    G = ledger.shape[0]
    n = G - g0 if n is None else n
    info = dict.fromkeys(abi.MONITOR_REPORT_FIELDS, 0)
    none = np.zeros(0, abi.MONITOR_EVENT_DTYPE)
    if g0 < 0 or n < 0 or g0 + n > G:
        return info, none, abi.RAFT_ERANGE
    if (max_events is not None and max_events < 0) or kinds & ~abi.MONITOR_ALL:
        return info, none, abi.RAFT_EINVAL
    hit = np.nonzero(ledger[g0:g0 + n, EVER if ever else NOW] & kinds)[0]
    room = len(hit) if max_events is None else min(int(max_events), len(hit))
    take = g0 + hit[:room]
    ev = np.zeros(room, abi.MONITOR_EVENT_DTYPE)
    ev["group"] = take
    for k, w in (("now", NOW), ("ever", EVER), ("down_since", DOWN_SINCE), ("stall_since", STALL_SINCE),
                 ("leader", LEADER), ("lag_mask", LAG_MASK)):
        ev[k] = ledger[take, w]
    info["delivered"], info["pending"], info["flagged"] = room, len(hit) - room, len(hit)
    return info, ev, abi.RAFT_OK


def valid_ledger(ledger, R: int) -> bool:
    """raft_monitor_write's rule: known bits in now and ever, leader in -1..R-1, no lag_mask bit at or above R,
    outages, down_total, longest, max_lag and stall_mark >= 0, reserved words 0."""
    a = np.asarray(ledger, dtype=np.int64).reshape(-1, abi.MONITOR_WORDS)
    u = a & 0xFFFFFFFF
    return bool((((u[:, NOW] | u[:, EVER]) & ~abi.MONITOR_ALL) == 0).all() and (a[:, LEADER] >= -1).all()
                and (a[:, LEADER] < R).all() and ((u[:, LAG_MASK] >> R) == 0).all()
                and (a[:, [OUTAGES, DOWN_TOTAL, LONGEST, MAX_LAG, STALL_MARK]] >= 0).all()
                and not a[:, [RSV0, RSV1]].any())


def valid_availability(hist, outages: int, down_steps: int, reserved=(0, 0)) -> bool:
    """raft_monitor_set_availability's rule."""
    return bool((np.asarray(hist) >= 0).all()) and outages >= 0 and down_steps >= 0 and not any(reserved)


def outages_of(samples):
    """A scalar re-derivation for one group: `samples` is the sequence of
    (step, has_leader) its observes saw.  Returns (the lengths of the outages
    that ended, the step of the running outage's first sample or None)."""
    ended, since = [], None
    for s, led in samples:
        if not led:
            if since is None:
                since = s
        elif since is not None:
            ended.append(max(1, s - since))
            since = None
    return ended, since


# ---- crafted groups: one per rule and per non-case, R = 3, log_cap 16, each in
# three phases (a state, an observe at step CRAFTED_STEPS[k]) under
# CRAFTED_CFG, from the zero ledger unless CRAFTED_LEDGER0 names words.
# Expected: the now word after each phase, written out by hand; ever is their
# running OR, written out too.
CR, CCAP = 3, 16
CRAFTED_STEPS = (10, 14, 20)
CRAFTED_CFG = config(leaderless_steps=4, stalled_steps=6, lag_entries=4, churn_terms=2, churn_steps=4)
F_, L_ = abi.FOLLOWER, abi.LEADER


def _rep(term=1, role=F_, last=0, commit=None):
    return dict(term=term, role=role, last=last, commit=last if commit is None else commit)


_idle = [_rep(), _rep(), _rep()]                                       # nobody leads
_led = [_rep(1, L_), _rep(), _rep()]                                   # replica 0 leads term 1, nothing to commit


def _backlog(commit, leader=0, term=2):
    """Every log holds 8 entries; the leader has committed `commit` of them."""
    return [_rep(term, L_ if r == leader else F_, 8, commit if r == leader else 0) for r in range(3)]


# name: (phase 0, phase 1, phase 2, (now after each), (ever after each))
CRAFTED = {
    # no leader at all: down since step 10; age 0 is below leaderless_steps = 4, age 4 is at it, age 10 above
    "down_all": (_idle, _idle, _idle, (0, LL, LL), (0, LL, LL)),
    # down since step 9 on record; a leader at step 10: an outage of length 1 (bucket 0), never flagged
    "outage_len1": (_led, _led, _led, (0, 0, 0), (0, 0, 0)),
    # down at step 10, a leader at step 14: length 4 (bucket 2), ended at the very age that would have flagged it
    "outage_mid": (_idle, _led, _led, (0, 0, 0), (0, 0, 0)),
    # down at 10, flagged at 14, a leader at step 20: length 10 (bucket 3); ever keeps the bit
    "outage_long": (_idle, _idle, _led, (0, LL, 0), (0, LL, LL)),
    # replica 0 is still LEADER of term 2 beside replica 2, LEADER of term 3: L is 2
    "stale_leader": ([_rep(2, L_, 2), _rep(3, F_, 2), _rep(3, L_, 2)],) * 3 + ((0, 0, 0), (0, 0, 0)),
    # commit 2, 4, 6 of 8: the backlog advances at every observe, stall_since follows
    "backlog_advances": (_backlog(2), _backlog(4), _backlog(6), (0, 0, 0), (0, 0, 0)),
    # commit 2 of 8 throughout: stalled since step 10, age 4 is below stalled_steps = 6, age 10 is not
    "backlog_stuck": (_backlog(2), _backlog(2), _backlog(2), (0, 0, ST), (0, 0, ST)),
    # the mark is 5 at step 10; replica 1 takes over in term 3 with commit 3, then 5: never above the mark
    "new_leader_below": (_backlog(5), _backlog(3, 1, 3), _backlog(5, 1, 3), (0, 0, ST), (0, 0, ST)),
    # the backlog is committed at step 20: stall_since back to -1, the mark to 0
    "backlog_gone": (_backlog(2), _backlog(2), _backlog(8), (0, 0, 0), (0, 0, 0)),
    # replica 1 is 3 behind the leader (one below lag_entries = 4), then 4 (at it), then level
    "lag_edge": ([_rep(1, L_, 6), _rep(1, F_, 3), _rep(1, F_, 6)], [_rep(1, L_, 6), _rep(1, F_, 2), _rep(1, F_, 6)],
                 [_rep(1, L_, 6), _rep(1, F_, 6), _rep(1, F_, 6)], (0, LAG, 0), (0, LAG, LAG)),
    # the lagging replica is the stale leader of term 2, 4 behind replica 1 of term 3
    "lag_stale_leader": ([_rep(2, L_, 1), _rep(3, L_, 5), _rep(3, F_, 5)],) * 3 + ((LAG, LAG, LAG), (LAG, LAG, LAG)),
    # T = 1, 3, 4: the window opens at (10, 1); at 14 the term rose by 2 and the window rolls over to (14, 3); at 20
    # the rise is 1 against the new window (it is 3 against the old)
    "churn_rolls": ([_rep(1, L_), _rep(1), _rep(1)], [_rep(3, L_), _rep(3), _rep(3)], [_rep(4, L_), _rep(4), _rep(4)],
                    (0, CH, 0), (0, CH, CH)),
    # down since step 1000 on record and the step index went backwards: age 0 throughout, below leaderless_steps
    "backwards": (_idle, _idle, _idle, (0, 0, 0), (0, 0, 0)),
}
CRAFTED_NAMES = list(CRAFTED)
CRAFTED_LEDGER0 = {"outage_len1": {DOWN_SINCE: 9}, "backwards": {DOWN_SINCE: 1000}}
# selected ledger words after phase 2: name -> {word: value}
CRAFTED_WORDS = {
    "down_all": {FIRST: 14, LEADER: -1, DOWN_SINCE: 10, OUTAGES: 0},
    "outage_len1": {DOWN_SINCE: -1, OUTAGES: 1, DOWN_TOTAL: 1, LONGEST: 1, LEADER: 0, FIRST: 0},
    "outage_mid": {DOWN_SINCE: -1, OUTAGES: 1, DOWN_TOTAL: 4, LONGEST: 4},
    "outage_long": {FIRST: 14, DOWN_SINCE: -1, OUTAGES: 1, DOWN_TOTAL: 10, LONGEST: 10, LEADER: 0},
    "stale_leader": {LEADER: 2, STALL_SINCE: -1},
    "backlog_advances": {STALL_SINCE: 20, STALL_MARK: 6},
    "backlog_stuck": {FIRST: 20, STALL_SINCE: 10, STALL_MARK: 2},
    "new_leader_below": {FIRST: 20, STALL_SINCE: 10, STALL_MARK: 5, LEADER: 1},
    "backlog_gone": {STALL_SINCE: -1, STALL_MARK: 0},
    "lag_edge": {FIRST: 14, LAG_MASK: 0, MAX_LAG: 0},
    "lag_stale_leader": {FIRST: 10, LEADER: 1, LAG_MASK: 1, MAX_LAG: 4},
    "churn_rolls": {FIRST: 14, WIN_START: 20, WIN_TERM: 4},
    "backwards": {DOWN_SINCE: 1000, LEADER: -1},
}
# the availability totals after the three phases: lengths 1, 4 and 10
CRAFTED_AVAIL = {"hist": {0: 1, 2: 1, 3: 1}, "outages": 3, "down_steps": 15}


def build(groups, R: int):
    """The state words of a list of groups, each a list of R _rep dicts."""
    w = blank_groups(len(groups), R)
    for g, reps in enumerate(groups):
        one = w[g:g + 1]
        for r, x in enumerate(reps):
            for k in ("term", "role", "commit", "last"):
                set_fld(one, R, r, k, x[k])
            set_fld(one, R, r, "phys", x["last"])
    return w


def crafted_phase(k: int) -> np.ndarray:
    return build([CRAFTED[name][k] for name in CRAFTED_NAMES], CR)


def crafted_ledger0() -> np.ndarray:
    L = fresh(len(CRAFTED_NAMES))
    for name, words in CRAFTED_LEDGER0.items():
        for w, v in words.items():
            L[CRAFTED_NAMES.index(name), w] = v
    return L


def crafted_now(k: int) -> np.ndarray:
    return np.array([CRAFTED[name][3][k] for name in CRAFTED_NAMES], np.int32)


def crafted_ever(k: int) -> np.ndarray:
    return np.array([CRAFTED[name][4][k] for name in CRAFTED_NAMES], np.int32)


def crafted_avail() -> dict:
    a = zero_avail()
    for k, v in CRAFTED_AVAIL["hist"].items():
        a["hist"][k] = v
    a["outages"], a["down_steps"] = CRAFTED_AVAIL["outages"], CRAFTED_AVAIL["down_steps"]
    return a


# ---- groups built in numpy, never stepped (the G = 70,001 case), R = 3, under
# BULK_CFG, observed at BULK_STEPS: group g with g % 100 == 7 k + 3 shows kind k
# (0 none, 1 LEADERLESS, 2 COMMIT_STALLED, 3 LAGGING, 4 CHURNING, 5 all but
# LEADERLESS) at the second observe
BULK_CFG = config(leaderless_steps=2, stalled_steps=2, lag_entries=3, churn_terms=2, churn_steps=50)
BULK_STEPS = (5, 8)
BULK_NOW = (0, LL, ST, LAG, CH, ST | LAG | CH)


def bulk(G: int, R: int = 3):
    """(the state of phase 0, of phase 1, the now words expected after phase 1).  Every group in phase 0, and the
    others in phase 1 too: replica 0 leads term 2 over 4 committed entries everywhere."""
    base = [_rep(2, L_, 4), _rep(2, F_, 4), _rep(2, F_, 4)]
    p0 = [base, [_rep(2), _rep(2), _rep(2)], [_rep(2, L_, 6, 4), _rep(2, F_, 4), _rep(2, F_, 4)], base, base,
          [_rep(2, L_, 6, 4), _rep(2, F_, 4), _rep(2, F_, 4)]]
    p1 = [base, [_rep(2), _rep(2), _rep(2)], [_rep(2, L_, 6, 4), _rep(2, F_, 4), _rep(2, F_, 4)],
          [_rep(2, L_, 4), _rep(2, F_, 1), _rep(2, F_, 4)], [_rep(4, L_, 4), _rep(4, F_, 4), _rep(4, F_, 4)],
          [_rep(4, L_, 6, 4), _rep(4, F_, 3), _rep(4, F_, 4)]]
    pick = np.zeros(G, np.int64)
    for k in range(1, 6):
        pick[7 * k + 3::100] = k
    one0, one1 = build(p0, R), build(p1, R)
    return one0[pick], one1[pick], np.array(BULK_NOW, np.int32)[pick]
