"""Cases for the step kernel's election bookkeeping (raft_step.h Stepper::step:
phase T's busy branch and what it hands to V and D, the loop-carried heartbeat
sessions, the rare counters), with the preconditions that show each path ran,
stated on the ORACLE's states and counter rows alone.
tests/test_election_paths_cpu.py checks the preconditions on the CPU;
tests/test_gpu_election_paths.py runs the same cases on the engine against the
oracle (counter rows per step, full state, logs and digest) at launch lengths
1, 37 and 300.

Shapes: G = 2 * (64 // R) + 1 groups -- a full wave of the step kernel, a
second one and a partial one with dead lanes -- for 300 steps, with short
election timers and heavy leader-isolation churn, so that most steps have an
electing group, and a small log_cap, so that appends overflow it.  Group 0
starts from a crafted state: replica 0 is in a vote round with its election
timer still armed (no schedule of the reference leaves that state, a
write_state does), so its timer fires while it is already electing.

A family is (R, log layout, protocol mode); its cases are the drop
thresholds 0, config 3's and 65,536 (drop_ppm 10^6: every message lost), each
on the kernel built for the workload and on the general one.  The layouts:
"flat" (every slot kept), "ring" (a log_window of log_cap slots: the ring
kernels, no access can miss, so the whole run is the oracle's) and
"ringmiss" (a window of half the log_cap, too small for the run on purpose:
the window-miss counters must count; the oracle's run is defined through the
first step that misses, and under this churn a ring that wraps misses within
a few steps, whatever its size).
"""
from __future__ import annotations

import functools

import numpy as np

import oracle as O
from helpers import abi, fld, set_fld

C = abi.C_INDEX
ARMED, ELECTING, PRST, HB, BACKOFF = (abi.FL_ARMED, abi.FL_ELECTING, abi.FL_PENDING_RST, abi.FL_HB_ACTIVE,
                                      abi.FL_BACKOFF)
PEND_SH = 8                     # include/raft_engine.h RAFT_FL_PENDING_SHIFT
STEPS = 300
LAUNCHES = (1, 37, 300)
P = 2000                        # heartbeat_ms: a step
TIMERS = dict(heartbeat_ms=P, election_min_ms=6000, election_max_ms=16000, backoff_min_ms=2000,
              backoff_max_ms=8000, round_timeout_ms=8000, retry_ms=4000)
LOG_CAP = 16
WINDOWS = {"flat": 0, "ring": 16, "ringmiss": 8}
DROPS = {"drop0": 0, "dropc3": abi.CONFIGS[3]["drop_ppm"], "dropall": 1_000_000}
SEEDS = {}                      # (R, layout, mode) -> seed, where the default (11) misses a path

# the paths every case with a working network must reach; with every message
# lost nobody is elected, so only the election-loop paths remain
ELECTION_PATHS = ("fire_while_electing", "two_senders", "backoff_restart")
ALL_PATHS = ELECTION_PATHS + ("backoff_end", "end_with_queued_reset", "stale_cancel", "start_in_d_ticked",
                              "log_overflow")


def groups_of(R):
    return 2 * (64 // R) + 1


def case_kw(R, layout, mode, drop):
    return dict(R=R, G=groups_of(R), seed=SEEDS.get((R, layout, mode), 11), log_cap=LOG_CAP,
                log_window=WINDOWS[layout], mode=mode, drop_ppm=DROPS[drop], churn_ppm=150_000, churn_steps=6,
                cmd_ppm=1_000_000, cmd_mode=abi.CMD_LOWEST_LEADER, **TIMERS)


def craft(state, R):
    """Group 0, replica 0: a candidate in its first vote round (every
    destination pending) whose election timer is armed and fires in the first
    step, before any response can end the round."""
    g = state[0:1]
    set_fld(g, R, 0, "role", abi.CANDIDATE)
    set_fld(g, R, 0, "term", 1)
    set_fld(g, R, 0, "voted", 1)
    set_fld(g, R, 0, "flags", ARMED | ELECTING | (((1 << R) - 1) << PEND_SH))
    set_fld(g, R, 0, "election_ms", P)
    set_fld(g, R, 0, "phase_ms", 0)
    set_fld(g, R, 0, "retry_ms", TIMERS["retry_ms"])
    return state


def start(kw, *targets):
    """The crafted start state into every target (oracle, engine)."""
    o = O.Oracle(abi.make_params(**kw))
    w = craft(o.read_state(), kw["R"])
    o.close()
    for x in targets:
        x.write_state(w)


def paths_of(before, after, row, R, kw):
    """Which paths one step took, from the oracle's state before and after it
    and its counter row.  Phase T runs first and reads only the replica's own
    fields, so its events are a function of the state before the step."""
    f = lambda w, name: np.stack([fld(w, R, r, name) for r in range(R)], -1).astype(np.int64)
    fl, el, ph, rty, role = f(before, "flags"), f(before, "election_ms"), f(before, "phase_ms"), \
        f(before, "retry_ms"), f(before, "role")
    fa, ra = f(after, "flags"), f(after, "role")
    armed, electing, backoff = (fl & ARMED) != 0, (fl & ELECTING) != 0, (fl & BACKOFF) != 0
    fire = armed & (el - P <= 0)
    start_fire = fire & ~electing
    # a fire makes the replica a CANDIDATE before its election clocks run
    role_t = np.where(fire, abi.CANDIDATE, role)
    in_round, in_bo = electing & ~backoff, electing & backoff
    pend = (fl >> PEND_SH) & 0xFF
    resend = in_round & (pend != 0) & (ph + P < kw["round_timeout_ms"]) & (rty - P <= 0)
    bo_end = in_bo & (ph - P <= 0)
    restart = bo_end & (role_t == abi.CANDIDATE)
    endel = bo_end & ~restart
    senders = start_fire | restart | resend
    ended = electing & ((fa & ELECTING) == 0)
    return {
        "fire_while_electing": bool((fire & electing).any()),
        "two_senders": bool((senders.sum(-1) >= 2).any()),
        "backoff_restart": bool(restart.any()),
        "backoff_end": bool(endel.any()),
        "end_with_queued_reset": bool((ended & ((fl & PRST) != 0)).any()),
        "stale_cancel": bool((((fl & HB) != 0) & ((fa & HB) == 0)).any()),
        # no session before the step, a LEADER with a session after it, and not
        # T's start (a backoff that ends as LEADER): D started the session.
        # The groups where that happened; oracle_run replays such a group alone
        # to see its own tick count (ticked_in_its_group)
        "start_in_d_ticked": np.nonzero((((fl & HB) == 0) & ((fa & HB) != 0) & (ra == abi.LEADER) &
                                         ~(bo_end & (role_t == abi.LEADER))).any(-1))[0],
        "log_overflow": int(row[C["log_overflow"]]) > 0,
        "log_window_miss": int(row[C["log_window_miss"]]) > 0,
    }


def ticked_in_its_group(kw, t, g, before, log, after):
    """Step t of group g alone (its state and logs before the step, its global
    id and the step index: every draw is keyed by them).  A heartbeat session
    that exists at phase A is either ticked or cancelled there, and FL_HB is
    set only before A (T, D), so the sessions the group ticks are exactly the
    ones it holds after the step: its own SESSIONS_TICKED must equal that
    count, the session D started included, and the replay must end in the
    state the whole run gave the group."""
    R = kw["R"]
    o = O.Oracle(abi.make_params(**dict(kw, G=1, g0=int(g))))
    o.write_state(before[g:g + 1])
    o.write_log(log[0][g:g + 1], log[1][g:g + 1])
    o.step_index = t
    row = o.step(1)[0, : abi.NUM_COUNTERS]
    same = np.array_equal(o.read_state(), after[g:g + 1])
    o.close()
    held = sum((int(fld(after[g], R, r, "flags")) & HB) != 0 for r in range(R))
    return same and int(row[C["leaders_elected"]]) >= 1 and int(row[C["sessions_ticked"]]) == held >= 1


@functools.lru_cache(maxsize=None)
def oracle_run(R, layout, mode, drop):
    """The oracle's run of a case, computed once and shared (never changed):
    counter rows [STEPS, NUM_COUNTERS], the digest after every step, the final
    state and logs, the steps at which each path ran, and the first step with a
    window miss (STEPS if none)."""
    kw = case_kw(R, layout, mode, drop)
    o = O.Oracle(abi.make_params(**kw))
    start(kw, o)
    rows, digests, hits = [], [], {}
    before = o.read_state()
    for t in range(STEPS):
        log = o.read_log()
        row = o.step(1)[0, : abi.NUM_COUNTERS].copy()
        after = o.read_state()
        for name, hit in paths_of(before, after, row, R, kw).items():
            if name == "start_in_d_ticked":
                hit = any(ticked_in_its_group(kw, t, g, before, log, after) for g in hit[:2])
            if hit:
                hits.setdefault(name, []).append(t)
        rows.append(row)
        digests.append(o.digest())
        before = after
    miss = hits.get("log_window_miss", [STEPS])[0]
    out = dict(kw=kw, rows=np.stack(rows), digests=digests, state=before, log=o.read_log(), hits=hits, first_miss=miss)
    o.close()
    return out


FAMILIES = [(R, layout, mode) for R in (3, 5, 7) for layout in WINDOWS
            for mode in (abi.MODE_REFERENCE, abi.MODE_TEXTBOOK)]


def family_id(fam):
    R, layout, mode = fam
    return f"R{R}-{layout}-{'textbook' if mode == abi.MODE_TEXTBOOK else 'reference'}"


CASES = [(*fam, drop, general) for fam in FAMILIES for drop in DROPS for general in (False, True)]


def case_id(case):
    return f"{family_id(case[:3])}-{case[3]}-{'general' if case[4] else 'built'}"
