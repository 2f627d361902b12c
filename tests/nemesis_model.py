"""Scripted network faults restated in plain Python over read_state /
write_state arrays (include/raft_engine.h, raft_isolate_batch,
raft_engine_heal_network, raft_engine_list_isolated): the reference of
test_nemesis_cpu.py (over the oracle) and test_gpu_nemesis.py (against the
engine's kernels).  Word 0 of a group's RAFT_GROUP_EXTRA (state[g, -2]) is the
isolation word, rem << 8 | replica.  Nothing here calls the engine."""
from __future__ import annotations

import numpy as np

import audit_model as AM
from helpers import abi, fld
from read_model import newest_leader
from sm_model import leader_of

SET, BUSY, NO_LEADER, DUPLICATE, INVALID = (abi.ISOLATE_SET, abi.ISOLATE_BUSY, abi.ISOLATE_NO_LEADER,
                                            abi.ISOLATE_DUPLICATE, abi.ISOLATE_INVALID)
NEWEST, LOWEST = abi.ISOLATE_NEWEST_LEADER, abi.ISOLATE_LOWEST_LEADER
ISO = -2                                 # the isolation word's place in a group's canonical words


def running(word: int) -> int:
    """Steps left of an isolation word, 0 if it is not running."""
    return max(int(word) >> 8, 0)


def in_range(target: int, steps: int, R: int) -> bool:
    return LOWEST <= target < R and 1 <= steps <= abi.ISOLATE_MAX_STEPS


def isolate(state, groups, targets, steps, R: int, replace: bool = False):
    """raft_isolate_batch over a whole engine's `state` [G, words], in place:
    (tickets, return code); (None, RAFT_ERANGE) when a group is outside the
    engine (nothing is written).  Per group the in-range message at the lowest
    batch position is judged, against the state before the call."""
    groups = np.asarray(groups, dtype=np.int64)
    targets = np.broadcast_to(np.asarray(targets, dtype=np.int32), groups.shape)
    steps = np.broadcast_to(np.asarray(steps, dtype=np.int32), groups.shape)
    if len(groups) and (groups.min() < 0 or groups.max() >= state.shape[0]):
        return None, abi.RAFT_ERANGE
    tickets = np.zeros(len(groups), dtype=abi.ISOLATE_TICKET_DTYPE)
    winner = {}
    for m, (g, want, st) in enumerate(zip(groups.tolist(), targets.tolist(), steps.tolist())):
        if not in_range(want, st, R):
            tickets[m] = (-1, st, INVALID, 0)
        elif g in winner:
            tickets[m] = (-1, st, DUPLICATE, winner[g])
        else:
            winner[g] = m
            word = int(state[g, ISO])
            rep = want if want >= 0 else newest_leader(state, R, g) if want == NEWEST else leader_of(state, R, g)
            if rep < 0:
                tickets[m] = (-1, st, NO_LEADER, word)
            elif running(word) and not replace:
                tickets[m] = (rep, st, BUSY, word)
            else:
                state[g, ISO] = st << 8 | rep
                tickets[m] = (rep, st, SET, word)
    return tickets, abi.RAFT_OK


def heal(state, R: int, mask=None, g0: int = 0, n=None) -> dict:
    """raft_engine_heal_network of groups [g0, g0 + n) of `state`, in place: the info."""
    n = (state.shape[0] - g0 if mask is None else len(mask)) if n is None else n
    info = dict.fromkeys(abi.HEAL_INFO_FIELDS, 0)
    for j in range(n):
        word = int(state[g0 + j, ISO])
        if not running(word):
            info["idle"] += 1
        elif mask is None or (int(mask[j]) >> (word & 0xFF)) & 1:
            state[g0 + j, ISO] = 0
            info["healed"] += 1
        else:
            info["kept"] += 1
    return info


def list_isolated(state, R: int, g0: int = 0, n=None, max_events=None):
    """raft_engine_list_isolated of groups [g0, g0 + n): (info, records)."""
    n = state.shape[0] - g0 if n is None else n
    rows = []
    for g in range(g0, g0 + n):
        word = int(state[g, ISO])
        if running(word):
            rep = word & 0xFF
            rows.append((g, rep, int(fld(state, R, rep, "role")[g]) if rep < R else -1, word >> 8))
    room = len(rows) if max_events is None else min(int(max_events), len(rows))
    info = dict(delivered=room, pending=len(rows) - room, running=len(rows))
    return info, np.array(rows[:room], dtype=abi.ISOLATED_DTYPE)


class Calls:
    """The three calls under RaftEngine's method names for any of the models'
    Hosts (the oracle as `o`): read_state -> the model above -> write_state."""

    def isolate(self, groups, targets, steps, replace: bool = False):
        st = self.o.read_state()
        tk, rc = isolate(st, groups, targets, steps, self.R, replace)
        if rc == abi.RAFT_OK:
            self.o.write_state(st)
        self.last_status = rc
        return tk

    def heal_network(self, mask=None, g0: int = 0, n=None) -> dict:
        st = self.o.read_state()
        info = heal(st, self.R, mask, g0, n)
        self.o.write_state(st)
        return info

    def isolated(self, g0: int = 0, n=None, max_events=None, peek: bool = False):
        info, rec = list_isolated(self.o.read_state(), self.R, g0, n, 0 if peek else max_events)
        return info, rec


class Host(Calls, AM.Host):
    """audit_model's Host (the consumers' models, restart, install, audits) with the three calls."""


# ---- crafted groups of five: one per status of raft_isolate_batch, written by hand
CR = 5
CRAFTED_NAMES = ["fixed", "newest", "lowest", "no_leader", "busy", "expired", "target_R", "target_m3", "steps_0",
                 "steps_big", "rem1"]


def crafted():
    """(state, targets, steps, tickets without REPLACE, tickets with it).  Every
    group but "no_leader" has replica 1 as LEADER of term 2 and replica 3 as
    LEADER of term 4 (a deposed one and its successor)."""
    from helpers import blank_groups, set_fld
    n = len(CRAFTED_NAMES)
    g = {k: i for i, k in enumerate(CRAFTED_NAMES)}
    w = blank_groups(n, CR)
    for r in range(CR):
        set_fld(w, CR, r, "term", 4)
    set_fld(w, CR, 1, "term", 2)
    set_fld(w, CR, 1, "role", abi.LEADER)
    set_fld(w, CR, 3, "role", abi.LEADER)
    for r in (1, 3):
        set_fld(w[g["no_leader"]:g["no_leader"] + 1], CR, r, "role", abi.FOLLOWER)
    w[g["busy"], ISO] = 7 << 8 | 2
    w[g["rem1"], ISO] = 1 << 8 | 4                                 # running: it expires in the next step
    w[g["expired"], ISO] = 3                                       # no steps left: not running
    tgt = np.full(n, 0, np.int32)
    stp = np.full(n, 9, np.int32)
    tgt[g["newest"]], tgt[g["lowest"]], tgt[g["no_leader"]], tgt[g["busy"]] = NEWEST, LOWEST, NEWEST, LOWEST
    tgt[g["target_R"]], tgt[g["target_m3"]] = CR, -3
    stp[g["steps_0"]], stp[g["steps_big"]] = 0, abi.ISOLATE_MAX_STEPS + 1
    want = {k: (0, 9, SET, 0) for k in CRAFTED_NAMES}
    want["newest"], want["lowest"], want["no_leader"] = (3, 9, SET, 0), (1, 9, SET, 0), (-1, 9, NO_LEADER, 0)
    want["busy"], want["rem1"] = (1, 9, BUSY, 7 << 8 | 2), (0, 9, BUSY, 1 << 8 | 4)
    want["expired"] = (0, 9, SET, 3)
    want["target_R"] = want["target_m3"] = (-1, 9, INVALID, 0)
    want["steps_0"], want["steps_big"] = (-1, 0, INVALID, 0), (-1, abi.ISOLATE_MAX_STEPS + 1, INVALID, 0)
    forced = dict(want, busy=(1, 9, SET, 7 << 8 | 2), rem1=(0, 9, SET, 1 << 8 | 4))
    rows = lambda d: np.array([d[k] for k in CRAFTED_NAMES], dtype=abi.ISOLATE_TICKET_DTYPE)
    return w, tgt, stp, rows(want), rows(forced)


def contended_batch(G: int, R: int, n: int, seed: int = 0):
    """(groups, targets, steps): n messages over G groups with many duplicates
    per group, every kind of target and a few out-of-range ones."""
    rng = np.random.default_rng(1000 * n + 10 * R + seed)
    groups = rng.integers(0, G, n, dtype=np.int64)
    targets = rng.integers(-3, R + 1, n).astype(np.int32)           # -3 and R are INVALID
    steps = rng.integers(0, 40, n).astype(np.int32)                 # 0 is INVALID
    return groups, targets, steps
