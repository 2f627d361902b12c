"""Scenarios for the leader tick's rare paths (raft_step.h Stepper::tick), with
the preconditions that show each path ran, stated on the ORACLE's states and
counter rows alone.  tests/test_tick_paths_cpu.py checks the preconditions on
the CPU; tests/test_gpu_tick_paths.py runs the same scenarios on the engine in
lockstep with the oracle (counters, state, logs, digest, every step).

A scenario is a dict: kw (raft_params overrides), steps, an optional setup
(state, terms, cmds) -> None that crafts the start state, and check(trace),
where trace = [(state_before, state_after, counter_row)] per step.
"""
from __future__ import annotations

import numpy as np

from helpers import abi, blank_groups, fld, set_fld, set_session

NF = abi.NUM_FIELDS
C = abi.C_INDEX
HB, ARMED, ELECTING = abi.FL_HB_ACTIVE, abi.FL_ARMED, abi.FL_ELECTING
FAR = 10 ** 9
QUIET = dict(election_min_ms=20000, election_max_ms=20000, backoff_min_ms=2000, backoff_max_ms=2000)


def nx_row(w, R, s):
    return np.stack([w[:, R * NF + s * R + d] for d in range(R)], -1)


def mc_row(w, R, s):
    return np.stack([w[:, R * NF + R * R + s * R + d] for d in range(R)], -1)


def run_oracle(o, steps):
    trace = []
    for _ in range(steps):
        before = o.read_state()
        row = o.step(1)[0, : abi.NUM_COUNTERS]
        trace.append((before, o.read_state(), row))
    return trace


def settled_single_leader(w, R, P=2000):
    """Per group: the replica whose session is the only one that ticks this
    step, in a group where phases T, V and D change nothing (nobody electing,
    no timer fires), so the state before the step is the state phase A sees;
    -1 elsewhere."""
    fl = np.stack([fld(w, R, r, "flags") for r in range(R)], -1)
    role = np.stack([fld(w, R, r, "role") for r in range(R)], -1)
    el = np.stack([fld(w, R, r, "election_ms") for r in range(R)], -1)
    hb = (fl & HB) != 0
    calm = ~np.any((fl & ELECTING) != 0, -1) & ~np.any(((fl & ARMED) != 0) & (el <= P), -1)
    one = (hb.sum(-1) == 1) & calm
    s = np.argmax(hb, -1)
    lead = role[np.arange(len(w)), s] == abi.LEADER
    return np.where(one & lead, s, -1)


def tail_cache_misses(w, R):
    """Counts of the tick's three HBM reads past the 2-deep tail caches, and of
    ticks of a leader with an empty log and nextIndex 1, over the settled
    groups of one state: (leader log[prev], leader log[i-1], own log[prev],
    empty-leader requests)."""
    s = settled_single_leader(w, R)
    g = np.nonzero(s >= 0)[0]
    last = np.stack([fld(w, R, r, "last") for r in range(R)], -1)[g]
    out = np.zeros(4, np.int64)
    for sv in range(R):
        m = s[g] == sv
        if not m.any():
            continue
        i = nx_row(w, R, sv)[g][m]
        ll = last[m][:, sv : sv + 1]
        own = last[m]
        prev = i - 2
        ok = (prev >= -1) & (prev < ll)
        has = (prev >= -1) & (i <= ll)
        out[0] += np.count_nonzero(ok & (prev >= 0) & (prev < ll - 2))
        out[1] += np.count_nonzero(has & (i < ll))
        out[2] += np.count_nonzero(ok & (prev >= 0) & (prev < own - 2))
        out[3] += np.count_nonzero((ll == 0) & (i == 1))
    return out


# ---- (a) tail-cache misses: followers lagging by 3 or more entries ---------------
def catch_up(R, window):
    kw = dict(R=R, G=96, seed=41, log_cap=256, log_window=window, cmd_ppm=700_000, partition_period=24,
              partition_len=14, drop_ppm=50_000)

    def check(trace):
        tot = sum(tail_cache_misses(b, R) for b, _, _ in trace)
        assert (tot > 0).all(), f"no tail-cache miss of some kind ran: {tot.tolist()}"
        lag = max(int((np.stack([fld(b, R, r, "last") for r in range(R)], -1).max(-1) -
                       np.stack([fld(b, R, r, "last") for r in range(R)], -1).min(-1)).max()) for b, _, _ in trace)
        assert lag >= 3, lag
        assert sum(int(row[C["entries_acked"]]) for _, _, row in trace) > 0
        if window:
            # the ring wraps, and no access is below the window (the engine
            # keeps only the window: a miss is counted, its value undefined)
            assert max(int(fld(trace[-1][1], R, r, "phys").max()) for r in range(R)) > window
            assert sum(int(row[C["log_window_miss"]]) for _, _, row in trace) == 0
    return dict(kw=kw, steps=130 if window else 220, check=check)


# ---- (b) loss compares at the threshold's edges ----------------------------------
DROP_EDGES = {"thr0": 0, "thr1": 1, "thr65536": 1_000_000, "config3": abi.CONFIGS[3]["drop_ppm"]}


def drop_edge(name, general):
    ppm = DROP_EDGES[name]
    kw = dict(R=5, G=512, seed=3, log_cap=128, drop_ppm=ppm, cmd_ppm=250_000,
              kernel=abi.KERNEL_GENERAL if general else abi.KERNEL_AUTO)

    def check(trace):
        dropped = sum(int(row[C["msg_dropped"]]) for _, _, row in trace)
        sent = sum(int(row[C["append_sent"]]) for _, _, row in trace)
        acked = sum(int(row[C["entries_acked"]]) for _, _, row in trace)
        if ppm == 0:
            assert dropped == 0 and sent > 0 and acked > 0
        elif ppm == 1_000_000:
            # every message to another replica is lost: only the self acks remain
            assert dropped > 0 and sum(int(row[C["leaders_elected"]]) for _, _, row in trace) == 0
        else:
            assert dropped > 0 and sent > dropped and acked > 0
    return dict(kw=kw, steps=300 if ppm == 1 else 120, check=check)


# ---- (c) session ownership: swap, spill and cancel in one tick -------------------
def two_sessions(isolated):
    """R = 3, two groups of one wave.  Group 0 is K11 after its first step: the
    deposed leader 0 still holds its session, so its tick is the S-10 cancel.
    Group 1 has two leaders with a session each (replica 0 at term 2, replica
    1 at term 3) that cannot reach each other -- every message dropped, or
    replica 1 isolated -- so both tick in the first step: session 0 is
    swapped in from spill (no primary after write_state), then session 1 is
    swapped in and session 0 goes to spill.  The cancel and the first swap
    are the same tick round of the wave."""
    R = 3
    kw = dict(R=R, G=2, seed=77, log_cap=64, **QUIET)
    if not isolated:
        kw.update(drop_ppm=1_000_000)

    def setup(w, t, c):
        for g in (0, 1):
            for r in range(R):
                set_fld(w[g : g + 1], R, r, "voted", 1)
                set_fld(w[g : g + 1], R, r, "flags", ARMED)
                set_fld(w[g : g + 1], R, r, "election_ms", FAR)
        a = w[0:1]
        set_fld(a, R, 0, "term", 5); set_fld(a, R, 0, "flags", ARMED | HB); set_fld(a, R, 0, "election_ms", 20000)
        set_fld(a, R, 1, "term", 5); set_fld(a, R, 2, "term", 2)
        set_session(a, R, 0, [1, 1, 1], [0, 0, 0])
        b = w[1:2]
        for r, term in ((0, 2), (1, 3)):
            set_fld(b, R, r, "role", abi.LEADER); set_fld(b, R, r, "term", term); set_fld(b, R, r, "flags", HB)
            set_fld(b, R, r, "last", 2); set_fld(b, R, r, "phys", 2)
            t[1, r, :2] = term; c[1, r, :2] = [11 + r, 21 + r]
        set_fld(b, R, 2, "term", 2)
        set_session(b, R, 0, [1, 2, 1], [0, 0, 0])
        set_session(b, R, 1, [2, 1, 3], [0, 0, 0])
        if isolated:
            b[0, R * NF + 2 * R * R] = (40 << 8) | 1

    def check(trace):
        b0, a0, row0 = trace[0]
        assert fld(b0, R, 0, "role")[0] == abi.FOLLOWER and fld(b0, R, 0, "flags")[0] & HB      # the cancel
        assert not fld(a0, R, 0, "flags")[0] & HB
        assert row0[C["sessions_ticked"]] == 2                                                 # both of group 1
        for r in (0, 1):
            assert fld(a0, R, r, "role")[1] == abi.LEADER and fld(a0, R, r, "flags")[1] & HB
        assert not np.array_equal(nx_row(a0, R, 0)[1], nx_row(b0, R, 0)[1]) or \
            not np.array_equal(mc_row(a0, R, 0)[1], mc_row(b0, R, 0)[1])                       # the spilled row changed
        assert trace[1][2][C["sessions_ticked"]] == 2
    return dict(kw=kw, steps=12, setup=setup, check=check)


# ---- (d) step-down and the commit replay -----------------------------------------
def step_down_and_replay():
    """R = 3, three groups of one wave.  Group 0: K11, a response with a higher
    term deposes the leader in the tick.  Group 1: a leader with four entries
    whose commitIndex lags at 0 while every row acks entry 3: a majority ends
    above commitIndex + 1, so the replay commits three times in one tick (the
    closed form can commit once).  Group 2: a heartbeat's ack lowers a
    matchIndex (5 -> 2) in a tick that also acks an entry."""
    R = 3
    kw = dict(R=R, G=3, seed=78, log_cap=64, **QUIET)

    def setup(w, t, c):
        for g in range(3):
            x = w[g : g + 1]
            for r in range(R):
                set_fld(x, R, r, "voted", 1); set_fld(x, R, r, "term", 1)
                set_fld(x, R, r, "flags", ARMED); set_fld(x, R, r, "election_ms", FAR)
            set_fld(x, R, 0, "role", abi.LEADER); set_fld(x, R, 0, "flags", HB)
        a = w[0:1]
        set_fld(a, R, 0, "term", 2); set_fld(a, R, 1, "term", 5); set_fld(a, R, 1, "voted", 3); set_fld(a, R, 2, "term", 2)
        set_session(a, R, 0, [1, 1, 1], [0, 0, 0])
        b = w[1:2]
        for r in range(R):
            n = 4 if r == 0 else 3
            set_fld(b, R, r, "last", n); set_fld(b, R, r, "phys", n)
            t[1, r, :n] = 1; c[1, r, :n] = [31, 32, 33, 34][:n]
        set_session(b, R, 0, [4, 4, 4], [3, 3, 3])
        d = w[2:3]
        for r in range(R):
            n = 2 if r < 2 else 1
            set_fld(d, R, r, "last", n); set_fld(d, R, r, "phys", n)
            t[2, r, :n] = 1; c[2, r, :n] = [41, 42][:n]
        set_session(d, R, 0, [2, 3, 2], [1, 5, 1])

    def check(trace):
        b0, a0, row0 = trace[0]
        assert fld(a0, R, 0, "role")[0] == abi.FOLLOWER and fld(a0, R, 0, "term")[0] == 5        # stepped down
        assert fld(a0, R, 0, "commit")[1] == 3 and row0[C["commits"]] >= 3                        # the replay
        assert mc_row(b0, R, 0)[2, 1] == 5 and mc_row(a0, R, 0)[2, 1] == 2                         # a row went down
        assert row0[C["entries_acked"]] >= 3 + 2
    return dict(kw=kw, steps=10, setup=setup, check=check)


def start(sc, *targets):
    """Write the scenario's crafted start state to every target (oracle, engine)."""
    if "setup" not in sc:
        return
    kw = sc["kw"]
    w = blank_groups(kw["G"], kw["R"])
    t = np.zeros((kw["G"], kw["R"], kw["log_cap"]), np.int32)
    c = np.zeros((kw["G"], kw["R"], kw["log_cap"]), np.uint32)
    sc["setup"](w, t, c)
    for x in targets:
        x.write_state(w)
        x.write_log(t, c)


CATCH_UP = [(R, W) for R in (3, 5, 7) for W in (0, 64)]
SCENARIOS = {f"catchup-R{R}-{'ring' if W else 'flat'}": (lambda R=R, W=W: catch_up(R, W)) for R, W in CATCH_UP}
SCENARIOS.update({f"drop-{n}-{'general' if g else 'built'}": (lambda n=n, g=g: drop_edge(n, g))
                  for n in DROP_EDGES for g in (False, True)})
SCENARIOS.update({"sessions-dropall": lambda: two_sessions(False), "sessions-isolated": lambda: two_sessions(True),
                  "stepdown-replay": step_down_and_replay})
