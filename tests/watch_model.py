"""The leader watch restated in numpy over the canonical state words
(include/raft_engine.h, raft_engine_poll_leaders, raft_engine_read_watch /
write_watch): the reference of test_watch_cpu.py (over the oracle) and
test_gpu_watch.py (against the engine's kernels).  The model carries its own
`seen` array; nothing here touches a device."""
from __future__ import annotations

import functools

import numpy as np

import restart_model as RM
from helpers import abi, blank_groups, fld, set_fld
from read_model import newest_leader

KINDS = ("gained", "lost", "moved", "reterm")


def fresh(G: int) -> np.ndarray:
    """`seen` before the first report: [G, 2] of (-1, 0)."""
    s = np.zeros((G, 2), np.int32)
    s[:, 0] = -1
    return s


def current(state, R: int) -> np.ndarray:
    """[n, 2] (leader, term) of every group of `state`: read_model.newest_leader
    and that replica's currentTerm, (-1, 0) where no replica is LEADER."""
    out = fresh(state.shape[0])
    for g in range(state.shape[0]):
        r = newest_leader(state, R, g)
        if r >= 0:
            out[g] = (r, int(fld(state, R, r, "term")[g]))
    return out


def kind_of(leader: int, prev_leader: int) -> str:
    """The kind of a changed group: the four partition them."""
    if prev_leader < 0:
        return "gained"                                            # (a changed group with no leader before has one now)
    if leader < 0:
        return "lost"
    return "moved" if leader != prev_leader else "reterm"


def poll(state, seen, R: int, g0: int = 0, n=None, max_events=None, peek: bool = False, cur=None):
    """raft_engine_poll_leaders of groups [g0, g0 + n) over a whole engine's
    `state` [G, words] and the watch's `seen` [G, 2] (advanced in place for the
    groups whose events are returned): (info, events, return code).
    max_events None: room for everything; peek: out == NULL with max_events 0;
    cur: current(state, R) where the caller has it already."""
    G = state.shape[0]
    n = G - g0 if n is None else n
    info = dict.fromkeys(abi.WATCH_INFO_FIELDS, 0)
    none = np.zeros(0, abi.EVENT_DTYPE)
    if g0 < 0 or n < 0 or g0 + n > G:
        return info, none, abi.RAFT_ERANGE
    if max_events is not None and max_events < 0:
        return info, none, abi.RAFT_EINVAL
    cur = current(state[g0:g0 + n], R) if cur is None else cur[g0:g0 + n]
    changed = np.nonzero((cur != seen[g0:g0 + n]).any(axis=1))[0]
    for j in changed.tolist():
        info[kind_of(int(cur[j, 0]), int(seen[g0 + j, 0]))] += 1
    info["leaderless"] = int((cur[:, 0] < 0).sum())
    room = 0 if peek else len(changed) if max_events is None else min(int(max_events), len(changed))
    take = changed[:room]
    ev = np.zeros(room, abi.EVENT_DTYPE)
    ev["group"] = g0 + take
    ev["leader"], ev["term"] = cur[take, 0], cur[take, 1]
    ev["prev_leader"], ev["prev_term"] = seen[g0 + take, 0], seen[g0 + take, 1]
    seen[g0 + take] = cur[take]
    info["delivered"], info["pending"] = room, len(changed) - room
    return info, ev, abi.RAFT_OK


def valid_watch(pairs, R: int) -> bool:
    """raft_engine_write_watch's rule: every leader in -1..R-1, every term >= 0, a leader of -1 with term 0 only."""
    a = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    return bool(((a[:, 0] >= -1) & (a[:, 0] < R) & (a[:, 1] >= 0) & ((a[:, 0] >= 0) | (a[:, 1] == 0))).all())


def directory(state, R: int):
    """The leader directory a consumer of every event ends up with: (leader [G], term [G])."""
    cur = current(state, R)
    return cur[:, 0].copy(), cur[:, 1].copy()


class Host(RM.Host):
    """restart_model's Host (the oracle under RaftEngine's method names) with the watch."""

    def __init__(self, **kw):
        super().__init__(**kw)
        self.seen = fresh(self.G)

    def poll_leaders(self, g0: int = 0, n=None, max_events=None, peek: bool = False):
        info, ev, self.last_status = poll(self.o.read_state(), self.seen, self.R, g0, n, max_events, peek)
        return info, ev

    def read_watch(self, g0: int = 0, n=None):
        n = self.G - g0 if n is None else n
        return self.seen[g0:g0 + n].copy()

    def write_watch(self, seen, g0: int = 0):
        a = np.asarray(seen)
        if not valid_watch(a, self.R):
            raise ValueError("write_watch")
        self.seen[g0:g0 + len(a)] = a


# ---- crafted states: one group per situation, the expected records written out by hand
CR = 3
CRAFTED_NAMES = ["no_leader", "one_leader", "older_below", "equal_terms", "re_elected", "leader_lost", "unchanged"]


def crafted():
    """(state, seen) of 7 groups of 3 replicas, every replica in term 3 unless said otherwise:
      no_leader     nobody leads; never reported: no event
      one_leader    replica 1 leads term 3; never reported: gained
      older_below   replica 0 is still LEADER in term 2, replica 2 leads term 3; the watch
                    reported (0, 2): moved to replica 2 -- the deposed leader at the lower
                    index does not shadow its successor
      equal_terms   replicas 1 and 2 are LEADER in term 3; never reported: gained, the lower index
      re_elected    replica 1 leads term 5; the watch reported (1, 3): reterm
      leader_lost   nobody leads; the watch reported (2, 3): lost
      unchanged     replica 0 leads term 3; the watch reported (0, 3): no event"""
    R, G = CR, len(CRAFTED_NAMES)
    g = {n: i for i, n in enumerate(CRAFTED_NAMES)}
    w = blank_groups(G, R)
    for r in range(R):
        set_fld(w, R, r, "term", 3)
    one = lambda name: w[g[name]:g[name] + 1]
    set_fld(one("one_leader"), R, 1, "role", abi.LEADER)
    set_fld(one("older_below"), R, 0, "role", abi.LEADER)
    set_fld(one("older_below"), R, 0, "term", 2)
    set_fld(one("older_below"), R, 2, "role", abi.LEADER)
    set_fld(one("equal_terms"), R, 1, "role", abi.LEADER)
    set_fld(one("equal_terms"), R, 2, "role", abi.LEADER)
    set_fld(one("re_elected"), R, 1, "role", abi.LEADER)
    set_fld(one("re_elected"), R, 1, "term", 5)
    set_fld(one("unchanged"), R, 0, "role", abi.LEADER)
    seen = fresh(G)
    seen[g["older_below"]] = (0, 2)
    seen[g["re_elected"]] = (1, 3)
    seen[g["leader_lost"]] = (2, 3)
    seen[g["unchanged"]] = (0, 3)
    return w, seen


# (group, leader, term, prev_leader, prev_term)
CRAFTED_EVENTS = np.array([(1, 1, 3, -1, 0), (2, 2, 3, 0, 2), (3, 1, 3, -1, 0), (4, 1, 5, 1, 3), (5, -1, 0, 2, 3)],
                          dtype=abi.EVENT_DTYPE)
CRAFTED_INFO = dict(delivered=5, pending=0, gained=2, lost=1, moved=1, reterm=1, leaderless=2)
CRAFTED_SEEN_AFTER = np.array([(-1, 0), (1, 3), (2, 3), (1, 3), (1, 5), (-1, 0), (0, 3)], dtype=np.int32)


def crafted_single():
    """(state, seen) of 3 groups of one replica (R = 1): a FOLLOWER never
    reported; a LEADER of term 2 never reported (gained); a LEADER of term 4
    reported as (0, 2) (reterm)."""
    w = blank_groups(3, 1)
    set_fld(w, 1, 0, "term", 2)
    set_fld(w[1:], 1, 0, "role", abi.LEADER)
    set_fld(w[2:], 1, 0, "term", 4)
    seen = fresh(3)
    seen[2] = (0, 2)
    return w, seen


CRAFTED_SINGLE_EVENTS = np.array([(1, 0, 2, -1, 0), (2, 0, 4, 0, 2)], dtype=abi.EVENT_DTYPE)
CRAFTED_SINGLE_INFO = dict(delivered=2, pending=0, gained=1, lost=0, moved=0, reterm=1, leaderless=1)


# ---- the parity scenario shared by test_watch_cpu.py (coverage, on the oracle
# alone) and test_gpu_watch.py (the engine against it)
PARITY_CASES = RM.PARITY_CASES
# restart_model.parity_kw's seed 11 and these steps meet test_watch_cpu.py's coverage condition on the oracle
PARITY_SEED = 11
WARM_STEPS, SETTLE_STEPS, RUN_ON_STEPS, DOWN_STEPS = 40, 3, 20, 6


def parity_kw(R: int, G: int, variant: str) -> dict:
    return dict(RM.parity_kw(R, G, variant), seed=PARITY_SEED)


def parity_run(x, label: str = "", poll: bool = True) -> list:
    """The scenario on `x` (a Host or a RaftEngine): 40 steps, a poll over
    [3, G - 2), 3 steps, a poll, a restart of restart_model.parity_mask over
    [3, G - 2) with down_steps, 20 steps, a poll over everything.  Returns the
    checkpoints, each a dict of everything that must be equal between the
    engine and the model; poll=False leaves the polls out (the engine that
    never polled)."""
    out = []
    g0, n = 3, max(x.G - 5, 0)

    def snap(what, counters, g0, n):
        p = dict(what=f"{label} {what}", counters=counters, state=x.read_state(), digest=x.digest())
        if poll:
            p["info"], p["events"] = x.poll_leaders(g0, n)
            p["watch"] = x.read_watch()
        out.append(p)

    snap("warm-up", x.step(WARM_STEPS), g0, n)
    snap("settle", x.step(SETTLE_STEPS), g0, n)
    x.restart(RM.parity_mask(x.R, x.G, 0), g0=3, down_steps=DOWN_STEPS)
    snap("run-on", x.step(RUN_ON_STEPS), 0, x.G)
    return out


@functools.lru_cache(maxsize=None)
def host_parity_run(R: int, G: int, variant: str, g0: int = 0):
    """parity_run on the oracle, once per input and shared.  Treat it as read-only."""
    h = Host(**parity_kw(R, G, variant), **({"g0": g0} if g0 else {}))
    points = parity_run(h, f"R{R} G{G} {variant}")
    h.close()
    return points


def cuts(total: int):
    """The max_events of the cut tests: one, around a wave of 64, all but one, all."""
    return sorted({m for m in (1, 63, 64, 65, total - 1, total) if 1 <= m <= total})


def drain(x, g0: int, n: int, max_events: int):
    """Poll [g0, g0 + n) of `x` with room for max_events until nothing is
    pending: (the infos, the event arrays, the watch after each poll)."""
    infos, events, watches = [], [], []
    while True:
        info, ev = x.poll_leaders(g0, n, max_events)
        infos.append(info)
        events.append(ev)
        watches.append(x.read_watch())
        if info["pending"] == 0:
            return infos, events, watches
        assert info["delivered"] == max_events and len(infos) < 10_000
