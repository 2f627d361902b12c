"""Leader no-op entries restated in numpy over the canonical state words and
logs (include/raft_engine.h, raft_engine_append_noops, raft_engine_sm_set_noop):
the reference of test_noop_cpu.py (over the oracle) and test_gpu_noop.py
(against the engine's kernels).  The append itself is the oracle's
append_command.  Nothing here touches a device."""
from __future__ import annotations

import functools

import numpy as np

import client_model as CM
import read_model as RD
import sm_model as M
import transfer_model as TM
from helpers import TIMER_SETS, abi, blank_groups, fld, set_fld
from read_model import newest_leader
from transfer_model import last_terms

ACCEPTED, GHOSTED, NO_LEADER, LOG_FULL, CURRENT = (abi.PROPOSE_ACCEPTED, abi.PROPOSE_GHOSTED, abi.PROPOSE_NO_LEADER,
                                                   abi.PROPOSE_LOG_FULL, abi.PROPOSE_CURRENT)
NOOP = 0xFFFF0001                       # the command id the scenarios use for the entry


def append_noops(o, g0: int, n: int, cmd: int, textbook: bool = False, W: int = 0):
    """raft_engine_append_noops of groups [g0, g0 + n) on the oracle `o`:
    (info, tickets, ticket_cmds, return code).  The leader, its term and the
    term of its last entry are read from the state and logs the call finds;
    the statuses of an append follow raft_propose_batch's rules for one
    message (client_model.propose), and the oracle's state afterwards must
    agree with them."""
    st = o.read_state()
    terms, cmds = o.read_log()
    R, cap = o.R, o.cap
    lt = last_terms(st, terms, R)
    info = dict.fromkeys(abi.NOOP_INFO_FIELDS, 0)
    tickets = np.zeros(n, dtype=abi.TICKET_DTYPE)
    tcmd = np.zeros(n, dtype=np.uint32)
    miss = 0
    grew = []
    for j in range(n):
        g = g0 + j
        L = newest_leader(st, R, g)
        if L < 0:
            tickets[j] = (-1, -1, 0, NO_LEADER)
            info["no_leader"] += 1
            continue
        T, last, phys = (int(fld(st, R, L, f)[g]) for f in ("term", "last", "phys"))
        if last >= 1 and lt[g, L] == T:
            tickets[j] = (L, last - 1, T, CURRENT)
            tcmd[j] = cmds[g, L, last - 1]
            info["current"] += 1
            continue
        if textbook:                                               # an array log: slot lastIndex is written
            status = LOG_FULL if last >= cap else ACCEPTED
            miss += status == ACCEPTED and bool(W) and last < phys - W
        else:                                                      # Commons.kt:58-61: appended at the physical end (Q1)
            status = LOG_FULL if phys >= cap else GHOSTED if phys != last else ACCEPTED
        tickets[j] = (L, last, T, status)
        tcmd[j] = cmd
        o.append_command(g, L, cmd)
        info["log_full"] += status == LOG_FULL
        info["ghosted"] += status == GHOSTED
        if status != LOG_FULL:
            info["appended"] += 1
            grew.append((g, L, last + 1))
    after = o.read_state()
    for g, L, last in grew:
        assert fld(after, R, L, "last")[g] == last, (g, L, last)
    return {k: int(v) for k, v in info.items()}, tickets, tcmd, (abi.RAFT_EWINDOW if miss else abi.RAFT_OK)


def sm_apply(state, terms, cmds, mach: M.Machine, R, cap, W=0, g0=0, n=None, replica=-1, noop=None) -> dict:
    """sm_model.apply with raft_engine_sm_set_noop: an entry whose cmd is `noop`
    counts and hashes like any other and writes no register (None: disabled,
    sm_model.apply itself)."""
    if noop is None:
        return M.apply(state, terms, cmds, mach, R, cap, W, g0, n, replica)
    n = state.shape[0] - g0 if n is None else n
    applied = lost = regressed = 0
    for g in range(g0, g0 + n):
        for r in (range(R) if replica < 0 else (replica,)):
            commit, last, phys = (int(fld(state, R, r, f)[g]) for f in ("commit", "last", "phys"))
            hi = min(max(min(commit, last), 0), cap)
            lo = int(mach.applied[g, r])
            if W:
                wl = max(0, phys - W)
                if wl > lo and hi > lo:
                    skip = min(wl, hi) - lo
                    lost += skip
                    mach.lost[g, r] += skip
                    lo += skip
                    mach.applied[g, r] = lo
            if hi < lo:
                regressed += 1
                continue
            h = int(mach.hash[g, r])
            for i in range(lo, hi):
                t, c = int(terms[g, r, i]), int(cmds[g, r, i])
                if c != noop:
                    mach.reg[g, r, c & (mach.S - 1)] = c
                h = (h * M.P + M.x_of(i, t, c)) & M.MASK
            mach.hash[g, r] = h
            applied += hi - lo
            mach.applied[g, r] = hi
    return {"applied": applied, "lost": lost, "regressed": regressed,
            "status": abi.RAFT_EWINDOW if lost else abi.RAFT_OK}


# ---- crafted states: one group per record kind of raft_engine_append_noops
CR, CCAP = 3, 8
CRAFTED_NAMES = ["no_leader", "empty", "older_tail", "own_tail", "two_leaders", "log_full", "ghost_tail"]


def crafted():
    """(state, terms, cmds) of 7 groups of 3 replicas, log_cap 8; unless said
    otherwise replica 1 leads term 3 and every replica holds entries of terms
    1 and 2 (cmd 100 g + 10 r + j):
      no_leader    nobody leads
      empty        every log is empty
      older_tail   as described: the tail is of term 2
      own_tail     the leader's tail is of term 3
      two_leaders  replica 0 is still LEADER in term 2, replica 2 leads term 3
      log_full     the leader's lastIndex = physLen = log_cap, every entry of term 2
      ghost_tail   the leader's physLen is 4 over lastIndex 2: reference mode
                   appends at the physical end (GHOSTED), textbook mode at 2"""
    R, G, cap = CR, len(CRAFTED_NAMES), CCAP
    g = {n: i for i, n in enumerate(CRAFTED_NAMES)}
    w = blank_groups(G, R)
    t = np.zeros((G, R, cap), np.int32)
    c = np.zeros((G, R, cap), np.uint32)
    for gi in range(G):
        for r in range(R):
            c[gi, r] = 100 * gi + 10 * r + np.arange(cap)
    t[:, :, 0], t[:, :, 1] = 1, 2
    for r in range(R):
        set_fld(w, R, r, "term", 3)
        set_fld(w, R, r, "last", 2)
        set_fld(w, R, r, "phys", 2)
    set_fld(w, R, 1, "role", abi.LEADER)
    one = lambda name: w[g[name]:g[name] + 1]
    set_fld(one("no_leader"), R, 1, "role", abi.FOLLOWER)
    for r in range(R):
        set_fld(one("empty"), R, r, "last", 0)
        set_fld(one("empty"), R, r, "phys", 0)
    t[g["own_tail"], 1, 1] = 3
    set_fld(one("two_leaders"), R, 1, "role", abi.FOLLOWER)
    set_fld(one("two_leaders"), R, 0, "role", abi.LEADER)
    set_fld(one("two_leaders"), R, 0, "term", 2)
    set_fld(one("two_leaders"), R, 2, "role", abi.LEADER)
    t[g["log_full"], 1, :] = 2
    set_fld(one("log_full"), R, 1, "last", cap)
    set_fld(one("log_full"), R, 1, "phys", cap)
    t[g["ghost_tail"], 1, 2:4] = 3                                 # stale slots beyond lastIndex: not the tail
    set_fld(one("ghost_tail"), R, 1, "phys", 4)
    return w, t, c


def crafted_want(textbook: bool):
    """(tickets, ticket_cmds, info) the crafted groups must get, written out by hand."""
    ghost = (1, 2, 3, ACCEPTED if textbook else GHOSTED)
    tk = np.array([(-1, -1, 0, NO_LEADER), (1, 0, 3, ACCEPTED), (1, 2, 3, ACCEPTED), (1, 1, 3, CURRENT),
                   (2, 2, 3, ACCEPTED), (1, CCAP, 3, LOG_FULL), ghost], dtype=abi.TICKET_DTYPE)
    cmds = np.array([0, NOOP, NOOP, 100 * 3 + 10 * 1 + 1, NOOP, NOOP, NOOP], dtype=np.uint32)
    info = dict(appended=4, current=1, no_leader=1, log_full=1, ghosted=0 if textbook else 1)
    return tk, cmds, info


RING_W, RING_CAP = 8, 32


def crafted_ring(textbook: bool):
    """(state, terms, cmds) of 2 groups of 3 in an 8-slot ring (log_cap 32),
    replica 1 leading term 3 over entries of term 2:
      0  lastIndex = physLen = 12: the window has wrapped, the append lands in slot 12 & 7
      1  textbook mode: lastIndex 2 under physLen 12, the add at 2 is below the window
         (12 - 8 = 4), RAFT_EWINDOW.  Reference mode, whose add always lands at the
         physical end: lastIndex = physLen = 9, wrapped by one slot"""
    R, cap = CR, RING_CAP
    w = blank_groups(2, R)
    t = np.full((2, R, cap), 2, np.int32)
    c = np.zeros((2, R, cap), np.uint32)
    for r in range(R):
        set_fld(w, R, r, "term", 3)
        set_fld(w, R, r, "last", 12)
        set_fld(w, R, r, "phys", 12)
    set_fld(w, R, 1, "role", abi.LEADER)
    if textbook:
        set_fld(w[1:2], R, 1, "last", 2)
    else:
        for r in range(R):
            set_fld(w[1:2], R, r, "last", 9)
            set_fld(w[1:2], R, r, "phys", 9)
    return w, t, c


def crafted_ring_want(textbook: bool):
    tk = np.array([(1, 12, 3, ACCEPTED), (1, 2 if textbook else 9, 3, ACCEPTED)], dtype=abi.TICKET_DTYPE)
    info = dict(appended=2, current=0, no_leader=0, log_full=0, ghosted=0)
    return tk, np.full(2, NOOP, np.uint32), info, (abi.RAFT_EWINDOW if textbook else abi.RAFT_OK)


class Host(TM.Host):
    """transfer_model's Host (the oracle under RaftEngine's method names) with
    the client path, the read path's begin and the no-op call."""

    @property
    def textbook(self) -> bool:
        return self.kw.get("mode", 0) == abi.MODE_TEXTBOOK

    def append_noops(self, g0: int = 0, n=None, cmd: int = NOOP, tickets: bool = False):
        n = self.G - g0 if n is None else n
        info, tk, tc, self.last_status = append_noops(self.o, g0, n, cmd, self.textbook, self.W)
        return (info, tk, tc) if tickets else info

    def propose(self, groups, cmds):
        tk, self.last_status = CM.propose(self.o, groups, cmds, self.textbook, self.W)
        return tk

    def resolve(self, groups, tickets, cmds, check: bool = True):
        out, self.last_status = CM.resolve(self.o.read_state(), *self.o.read_log(), groups, tickets, cmds, self.R,
                                           self.cap, self.W)
        return out

    def begin_reads(self, groups):
        tk, self.last_status = RD.begin(self.o.read_state(), self.o.read_log()[0], groups, self.R, self.cap, self.W)
        return tk

    def sm_apply(self, g0=0, n=None, replica=-1, noop=None) -> dict:
        return sm_apply(self.o.read_state(), *self.o.read_log(), self.mach, self.R, self.cap, self.W, g0, n, replica,
                        noop)

    def check_log_matching(self) -> int:
        from helpers import log_matching_flags
        return int(log_matching_flags(self.o.read_state(), *self.o.read_log(), self.R, self.W).sum())


# ---- the parity scenario shared by test_noop_cpu.py (non-vacuity, on the
# oracle alone) and test_gpu_noop.py (the engine against it)
PARITY_CASES = TM.PARITY_CASES


def parity_run(x, label: str = "") -> list:
    """The scenario on `x` (a Host or a RaftEngine): 40 steps, append_noops over
    [3, G - 2) with tickets, 3 steps, resolve, append_noops again, 20 steps.
    Returns the checkpoints, each a dict of everything that must be equal
    between the engine and the oracle."""
    out = []

    def snap(what, **more):
        out.append(dict(what=f"{label} {what}", state=x.read_state(), logs=x.read_log(), digest=x.digest(), **more))

    g0, n = 3, max(x.G - 5, 0)
    groups = np.arange(g0, g0 + n, dtype=np.int64)
    snap("warm-up", counters=x.step(40))
    info, tk, tc = x.append_noops(g0, n, NOOP, tickets=True)
    snap("noops", info=info, tickets=tk, cmds=tc, rc=x.last_status if n else abi.RAFT_OK)
    snap("settle", counters=x.step(3))
    snap("resolve", states=x.resolve(groups, tk, tc, check=False))
    info, tk, tc = x.append_noops(g0, n, NOOP, tickets=True)
    snap("again", info=info, tickets=tk, cmds=tc, rc=x.last_status if n else abi.RAFT_OK)
    snap("run-on", counters=x.step(20))
    return out


@functools.lru_cache(maxsize=None)
def host_parity_run(R: int, G: int, variant: str, g0: int = 0):
    """parity_run on the oracle, once per input and shared: (checkpoints, every
    counter row).  Treat it as read-only."""
    kw = TM.RM.parity_kw(R, G, variant)
    h = Host(**kw, **({"g0": g0} if g0 else {}))
    points = parity_run(h, f"R{R} G{G} {variant}")
    h.close()
    return points, np.concatenate([p["counters"] for p in points if "counters" in p])


def assert_same_points(got: list, want: list, R: int):
    """Every checkpoint of the engine's parity_run equals the oracle's, bit for
    bit, as long as the run is valid: on a ring, up to the first step in which
    the oracle counts a window miss (transfer_model.assert_same_points)."""
    from helpers import assert_same_logs, assert_same_state
    assert len(got) == len(want)
    for a, b in zip(got, want):
        label = b["what"]
        if "counters" in b and not TM.RM.assert_same_rows(a["counters"], b["counters"], label):
            return
        for k in ("tickets", "cmds", "states"):
            if k in b:
                assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), \
                    f"{label}: {k} differ at {np.nonzero(a[k] != b[k])[0][:5]}: {a[k][a[k] != b[k]][:3]} vs " \
                    f"{b[k][a[k] != b[k]][:3]}"
        for k in ("info", "rc"):
            assert a.get(k) == b.get(k), f"{label}: {k} {a.get(k)} vs {b.get(k)}"
        assert_same_state(a["state"], b["state"], R, label)
        assert_same_logs(a["state"], a["logs"], b["logs"], R, label)
        assert a["digest"] == b["digest"], f"{label}: digest differs with equal state and logs"


# ---- the liveness scenarios: an idle textbook engine without faults.  The timers are helpers.TIMER_SETS["odd"]:
# under the reference's (20-23 s timeouts over a 2 s heartbeat) split votes leave a third of 203 groups without
# a leader for hundreds of steps, under these every group has one by step 13
LIVE_KW = dict(R=5, G=203, seed=11, log_cap=64, mode=abi.MODE_TEXTBOOK, ae_max_entries=4, cmd_ppm=0,
               **TIMER_SETS["odd"])
LIVE_SLOTS = 8
STEP_LIMIT = 200                        # no wait below comes near it: the runs end or fail


def step_until(x, done, limit: int = STEP_LIMIT) -> int:
    """Step `x` one step at a time until done(counter row) holds; the steps taken."""
    for k in range(1, limit + 1):
        if done(x.step(1)[-1]):
            return k
    raise AssertionError(f"not reached within {limit} steps")


def all_led(x):
    return lambda row: row[abi.C_INDEX["groups_with_leader"]] == x.G


def idle_reads(x, settle=None) -> dict:
    """An idle engine: step until every group has a leader, begin a read in
    every group, append the no-ops, step `settle` steps (None: until every
    ticket resolves COMMITTED, and report how many that took), resolve, begin
    again.  Everything a Host and a RaftEngine must agree on."""
    groups = np.arange(x.G, dtype=np.int64)
    warm = step_until(x, all_led(x))
    before = x.begin_reads(groups)
    info, tk, tc = x.append_noops(0, x.G, NOOP, tickets=True)
    if settle is None:
        settle = 0
        while not (x.resolve(groups, tk, tc)["status"] == CM.COMMITTED).all():
            x.step(1)
            settle += 1
            assert settle < STEP_LIMIT
    else:
        x.step(settle)
    return dict(warm=warm, settle=settle, before=before, info=info, tickets=tk, cmds=tc,
                resolved=x.resolve(groups, tk, tc), after=x.begin_reads(groups), digest=x.digest())


def stalled_tickets(x, settle=None) -> dict:
    """The stalled-ticket case: once every group has a leader, an evacuate of
    replica 0 and a proposal to every group with no step in between (the
    proposal goes to the leader that is about to be replaced), then steps until
    every group that replica 0 led has a leader in a higher term, then 30 more.
    The tickets still PENDING then are the stalled ones: no later step commits
    them, for want of an entry of the new term.  append_noops, then `settle`
    steps (None: until none of them is PENDING, and report how many that took).
    Dual-leader counts and Log Matching are watched throughout."""
    groups = np.arange(x.G, dtype=np.int64)
    dual = 0

    def step(n):
        nonlocal dual
        rows = x.step(n)
        dual += int(rows[:, abi.C_INDEX["dual_leader_groups"]].sum())
        return rows

    warm = 0
    while True:
        warm += 1
        if step(1)[-1, abi.C_INDEX["groups_with_leader"]] == x.G:
            break
        assert warm < STEP_LIMIT
    led0 = np.nonzero(x.leaders()["leader"] == 0)[0]
    evac = x.evacuate(np.full(x.G, 1, np.uint8))
    cmds = (1000 + groups).astype(np.uint32)
    tk = x.propose(groups, cmds)
    moved = 0
    while True:
        moved += 1
        step(1)
        st = x.read_state()
        newest = np.array([max([int(fld(st, x.R, r, "term")[g]) for r in range(x.R)
                                if fld(st, x.R, r, "role")[g] == abi.LEADER], default=-1) for g in led0])
        if (newest > tk["term"][led0]).all():
            break
        assert moved < STEP_LIMIT
    step(30)
    later = x.resolve(groups, tk, cmds)
    stalled = np.nonzero(later["status"] == CM.PENDING)[0]
    matching = x.check_log_matching()
    info, ntk, ntc = x.append_noops(0, x.G, NOOP, tickets=True)
    if settle is None:
        settle = 0
        while (x.resolve(groups, tk, cmds)["status"][stalled] == CM.PENDING).any():
            step(1)
            settle += 1
            assert settle < STEP_LIMIT
    else:
        step(settle)
    final = x.resolve(groups, tk, cmds)
    return dict(warm=warm, moved=moved, settle=settle, led0=led0.tolist(), evacuate=evac, tickets=tk, later=later,
                stalled=stalled.tolist(), info=info, noop_tickets=ntk, final=final, dual=dual,
                matching=matching + x.check_log_matching(), digest=x.digest())


@functools.lru_cache(maxsize=None)
def host_idle_reads():
    h = Host(**LIVE_KW)
    out = idle_reads(h)
    h.close()
    return out


@functools.lru_cache(maxsize=None)
def host_stalled_tickets():
    h = Host(**LIVE_KW)
    out = stalled_tickets(h)
    h.close()
    return out
