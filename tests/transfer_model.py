"""Leadership transfer restated in numpy over the canonical state words
(include/raft_engine.h, raft_transfer_batch, raft_engine_resolve_transfers,
raft_engine_evacuate): the reference of test_transfer_cpu.py (over the oracle)
and test_gpu_transfer.py (against the engine's kernels).  Nothing here touches
a device."""
from __future__ import annotations

import functools

import numpy as np

import oracle as O
import restart_model as RM
from helpers import abi, blank_groups, fld, set_fld
from read_model import newest_leader

(SENT, NO_LEADER, SELF, BEHIND, BUSY, UNREACHABLE, NO_TARGET, INVALID) = (
    abi.TRANSFER_SENT, abi.TRANSFER_NO_LEADER, abi.TRANSFER_SELF, abi.TRANSFER_BEHIND, abi.TRANSFER_BUSY,
    abi.TRANSFER_UNREACHABLE, abi.TRANSFER_NO_TARGET, abi.TRANSFER_INVALID)
COMPLETED, PENDING, SUPERSEDED, NONE = (abi.TRANSFER_COMPLETED, abi.TRANSFER_PENDING, abi.TRANSFER_SUPERSEDED,
                                        abi.TRANSFER_NONE)
AUTO = abi.TRANSFER_AUTO
BUSY_FLAGS = abi.FL_ELECTING | abi.FL_BACKOFF | abi.FL_PENDING_RST


def last_terms(state, terms, R: int) -> np.ndarray:
    """[n, R]: the term of each replica's last entry, log[lastIndex - 1].term, 0 for an empty log."""
    n = state.shape[0]
    out = np.zeros((n, R), np.int32)
    for r in range(R):
        last = fld(state, R, r, "last")
        has = last >= 1
        out[has, r] = terms[np.nonzero(has)[0], r, last[has] - 1]
    return out


def isolated(word: int) -> int:
    """The replica a group's isolation word (rem << 8 | replica) cuts off, -1 if it is not running."""
    return (word & 0xFF) if (word >> 8) > 0 else -1


def judge(state, lt, R: int, g: int, r: int, lead: int) -> int:
    """Why replica r cannot take over from leader `lead` of group g: SENT if it
    can, else BEHIND, BUSY or UNREACHABLE, in that order."""
    if fld(state, R, r, "last")[g] != fld(state, R, lead, "last")[g] or lt[g, r] != lt[g, lead]:
        return BEHIND
    fl = int(fld(state, R, r, "flags")[g])
    if fld(state, R, r, "role")[g] != abi.FOLLOWER or not fl & abi.FL_ARMED or fl & BUSY_FLAGS:
        return BUSY
    if r == isolated(int(state[g, -2])):
        return UNREACHABLE
    return SENT


def choose(state, lt, R: int, g: int, lead: int, excluded: int = 0):
    """AUTO's choice: (the first replica after `lead`, cyclically, outside
    `excluded` that judge() lets through, or -1; the statuses the others got)."""
    seen = set()
    to = -1
    for k in range(1, R):
        r = (lead + k) % R
        if (excluded >> r) & 1:
            continue
        st = judge(state, lt, R, g, r, lead)
        if st != SENT:
            seen.add(st)
        elif to < 0:
            to = r
    return to, seen


def transfer(state, groups, targets, R: int, last_term=None):
    """raft_transfer_batch over a whole engine's `state` [G, words], in place;
    last_term [G, R] is last_terms() of its logs (None: every log ends in the
    same term).  Returns (tickets, return code); (None, RAFT_ERANGE) when a group
    is outside the engine (nothing is written).  Every message is judged against
    the state before the call."""
    groups = np.asarray(groups, dtype=np.int64)
    targets = np.full(len(groups), AUTO, np.int32) if targets is None else np.asarray(targets, dtype=np.int32)
    if len(groups) and (groups.min() < 0 or groups.max() >= state.shape[0]):
        return None, abi.RAFT_ERANGE
    lt = np.zeros((state.shape[0], R), np.int32) if last_term is None else last_term
    before = state.copy()
    tickets = np.zeros(len(groups), dtype=abi.TRANSFER_TICKET_DTYPE)
    for m, (g, want) in enumerate(zip(groups.tolist(), targets.tolist())):
        if not -1 <= want < R:
            tickets[m] = (-1, 0, -1, INVALID)
            continue
        lead = newest_leader(before, R, g)
        if lead < 0:
            tickets[m] = (-1, 0, -1, NO_LEADER)
            continue
        T = int(fld(before, R, lead, "term")[g])
        if want == lead:
            st, to = SELF, -1
        elif want >= 0:
            st, to = judge(before, lt, R, g, want, lead), want
        else:
            to, _ = choose(before, lt, R, g, lead)
            st = SENT if to >= 0 else NO_TARGET
        if st == SENT:
            state[g, to * abi.NUM_FIELDS + abi.F_INDEX["election_ms"]] = 1
        tickets[m] = (lead, T, to if st == SENT else -1, st)
    return tickets, abi.RAFT_OK


def resolve(state, groups, tickets, R: int):
    """raft_engine_resolve_transfers over `state` [G, words]: (records, return code)."""
    groups = np.asarray(groups, dtype=np.int64)
    out = np.zeros(len(groups), dtype=abi.TRANSFER_STATE_DTYPE)
    bad_g = bad_t = False
    for m, (g, tk) in enumerate(zip(groups.tolist(), tickets.tolist())):
        frm, T, to, st = tk
        if not 0 <= g < state.shape[0]:
            bad_g = True
            out[m] = (INVALID, -1, 0, 0)
        elif st != SENT:
            out[m] = (NONE, -1, 0, 0)
        elif not (0 <= frm < R and 0 <= to < R):
            bad_t = True
            out[m] = (INVALID, -1, 0, 0)
        else:
            above = [(int(fld(state, R, r, "term")[g]), -r) for r in range(R)
                     if fld(state, R, r, "role")[g] == abi.LEADER and fld(state, R, r, "term")[g] > T]
            if any(-nr == to for _, nr in above):
                out[m] = (COMPLETED, to, int(fld(state, R, to, "term")[g]), 0)
            elif above:
                t, nr = max(above)                                  # the newest: the highest term, the lowest id
                out[m] = (SUPERSEDED, -nr, t, 0)
            else:
                out[m] = (PENDING, -1, 0, 0)
    return out, (abi.RAFT_ERANGE if bad_g else abi.RAFT_EINVAL if bad_t else abi.RAFT_OK)


def evacuate(state, mask, R: int, g0: int = 0, last_term=None) -> dict:
    """raft_engine_evacuate of groups [g0, g0 + len(mask)) of a whole engine's
    `state`, in place; returns the info."""
    lt = np.zeros((state.shape[0], R), np.int32) if last_term is None else last_term
    info = dict.fromkeys(abi.EVACUATE_INFO_FIELDS, 0)
    before = state.copy()
    for j, mk in enumerate(np.asarray(mask, dtype=np.uint8).tolist()):
        g = g0 + j
        mk &= (1 << R) - 1
        lead = newest_leader(before, R, g)
        if lead < 0 or not (mk >> lead) & 1:
            continue
        info["led"] += 1
        to, seen = choose(before, lt, R, g, lead, mk)
        if to >= 0:
            info["sent"] += 1
            state[g, to * abi.NUM_FIELDS + abi.F_INDEX["election_ms"]] = 1
        else:
            info["no_target"] += 1
            info["behind"] += int(BEHIND in seen)
            info["busy"] += int(BUSY in seen or UNREACHABLE in seen)
    return info


def leaders(state, R: int) -> np.ndarray:
    """raft_engine_read_leaders over `state`: abi.LEADER_DTYPE records (the
    lowest replica index with role LEADER or -1, its term and commitIndex, the
    number of LEADERs)."""
    out = np.zeros(state.shape[0], dtype=abi.LEADER_DTYPE)
    out["leader"] = -1
    for g in range(state.shape[0]):
        ls = [r for r in range(R) if fld(state, R, r, "role")[g] == abi.LEADER]
        if ls:
            out[g] = (ls[0], int(fld(state, R, ls[0], "term")[g]), len(ls), int(fld(state, R, ls[0], "commit")[g]))
    return out


# ---- crafted states: one group per situation of raft_transfer_batch
EL = abi.F_INDEX["election_ms"]


def healthy(G: int, R: int, leader: int = 1):
    """(state, last_term): G groups in which replica `leader` leads term 3 and
    every other replica is an idle armed follower with the leader's log (4
    entries, the last of term 2)."""
    w = blank_groups(G, R)
    for r in range(R):
        set_fld(w, R, r, "term", 3)
        set_fld(w, R, r, "last", 4)
        set_fld(w, R, r, "phys", 4)
        set_fld(w, R, r, "flags", abi.FL_ARMED)
        set_fld(w, R, r, "election_ms", 20000 + r)
    set_fld(w, R, leader, "role", abi.LEADER)
    set_fld(w, R, leader, "flags", abi.FL_HB_ACTIVE)
    set_fld(w, R, leader, "election_ms", 0)
    return w, np.full((G, R), 2, np.int32)


def crafted():
    """(state, last_term, targets, expected tickets): one group of 5 per
    situation of raft_transfer_batch."""
    R = 5
    names = ["no_leader", "self", "shorter", "other_term", "electing", "candidate", "disarmed", "iso_target",
             "iso_other", "target_R", "target_m2", "stale_leader", "plain", "iso_expired", "backoff", "pending_rst",
             "longer"]
    w, lt = healthy(len(names), R)
    g = {n: slice(i, i + 1) for i, n in enumerate(names)}
    tgt = np.full(len(names), 2, np.int32)
    want = {n: (1, 3, -1, BUSY) for n in names}
    set_fld(w[g["no_leader"]], R, 1, "role", abi.FOLLOWER)
    want["no_leader"] = (-1, 0, -1, NO_LEADER)
    tgt[g["self"]] = 1
    want["self"] = (1, 3, -1, SELF)
    set_fld(w[g["shorter"]], R, 2, "last", 3)
    want["shorter"] = (1, 3, -1, BEHIND)
    lt[g["other_term"], 2] = 1
    want["other_term"] = (1, 3, -1, BEHIND)
    set_fld(w[g["longer"]], R, 2, "last", 5)
    set_fld(w[g["longer"]], R, 2, "phys", 5)
    want["longer"] = (1, 3, -1, BEHIND)
    set_fld(w[g["electing"]], R, 2, "flags", abi.FL_ARMED | abi.FL_ELECTING)
    set_fld(w[g["candidate"]], R, 2, "role", abi.CANDIDATE)
    set_fld(w[g["disarmed"]], R, 2, "flags", 0)
    set_fld(w[g["disarmed"]], R, 2, "election_ms", 0)
    set_fld(w[g["backoff"]], R, 2, "flags", abi.FL_ARMED | abi.FL_BACKOFF)
    set_fld(w[g["pending_rst"]], R, 2, "flags", abi.FL_ARMED | abi.FL_PENDING_RST)
    w[g["iso_target"], -2] = 3 << 8 | 2
    want["iso_target"] = (1, 3, -1, UNREACHABLE)
    w[g["iso_other"], -2] = 3 << 8 | 4
    want["iso_other"] = (1, 3, 2, SENT)
    w[g["iso_expired"], -2] = 2                                   # no steps left: not running
    want["iso_expired"] = (1, 3, 2, SENT)
    tgt[g["target_R"]], tgt[g["target_m2"]] = R, -2
    want["target_R"] = want["target_m2"] = (-1, 0, -1, INVALID)
    # replica 0 still LEADER in term 2 beside the newest, replica 1 in term 3: `from` is 1, and 0 as a target is BUSY
    set_fld(w[g["stale_leader"]], R, 0, "role", abi.LEADER)
    set_fld(w[g["stale_leader"]], R, 0, "term", 2)
    tgt[g["stale_leader"]] = 0
    want["plain"] = (1, 3, 2, SENT)
    return w, lt, tgt, np.array([want[n] for n in names], dtype=abi.TRANSFER_TICKET_DTYPE), names


class Host(RM.Host):
    """restart_model's Host (the oracle with the consumers' models beside it,
    under RaftEngine's method names) with the transfer calls: read_state ->
    the model above -> write_state.  `sent` counts the timers the calls set."""

    def __init__(self, slots: int = 0, **kw):
        super().__init__(slots, **kw)
        self.kw = dict(kw)
        self.sent = 0

    def reparam(self, **changes):
        """Go on under other raft_params (cmd_ppm, say): a new oracle that is
        given this one's state, logs and step index."""
        self.kw.update(changes)
        self.p = abi.make_params(**self.kw)
        o = O.Oracle(self.p)
        o.write_state(self.o.read_state())
        o.write_log(*self.o.read_log())
        o.step_index = self.o.step_index
        self.o.close()
        self.o = o

    def _whole(self):
        st = self.o.read_state()
        return st, last_terms(st, self.o.read_log()[0], self.R)

    def transfer(self, groups, targets=None):
        st, lt = self._whole()
        tk, rc = transfer(st, groups, targets, self.R, lt)
        if rc == abi.RAFT_OK:
            self.o.write_state(st)
            self.sent += int((tk["status"] == SENT).sum())
        self.last_status = rc
        return tk

    def resolve_transfers(self, groups, tickets, check: bool = True):
        out, self.last_status = resolve(self.o.read_state(), groups, tickets, self.R)
        return out

    def evacuate(self, mask, g0: int = 0) -> dict:
        st, lt = self._whole()
        info = evacuate(st, mask, self.R, g0, lt)
        self.o.write_state(st)
        self.sent += info["sent"]
        return info

    def leaders(self, g0: int = 0, n=None):
        return leaders(self.o.read_state(g0, n), self.R)


# ---- the parity scenario shared by test_transfer_cpu.py (non-vacuity, on the
# oracle alone) and test_gpu_transfer.py (the engine against it)

# restart_model's shapes and their reasons (a partial second wave, unaligned ends, R = 1 where every transfer is
# NO_TARGET or SELF), without (7, 10)
PARITY_SHAPES = [(3, 23), (5, 203), (8, 9), (1, 5), (1, 70)]
PARITY_CASES = [(R, G, v) for R, G in PARITY_SHAPES for v in ("flat", "ring") + (("textbook",) if R == 5 else ())]
EVACUATE_MASK = 0b101


def parity_messages(R: int, G: int):
    """(groups, targets): every group of [3, G - 2) once with a seeded target in
    -1..R-1, then 7 of them again (fewer where the range is shorter) with the
    next target, cyclically in -1..R-1."""
    rng = np.random.default_rng(1000 * R + G)
    g = np.arange(3, max(G - 2, 3), dtype=np.int64)
    t = rng.integers(-1, R, len(g)).astype(np.int32)
    dup = rng.permutation(len(g))[:7]
    return np.concatenate([g, g[dup]]), np.concatenate([t, ((t[dup] + 2) % (R + 1) - 1).astype(np.int32)])


def parity_run(x, label: str = "") -> list:
    """The scenario on `x` (a Host or a RaftEngine): 40 steps, the transfer
    batch, 3 steps, resolve, evacuate of replicas 0 and 2 over [3, G - 2), 40
    steps.  Returns the checkpoints, each a dict of everything that must be
    equal between the engine and the oracle."""
    out = []

    def snap(what, **more):
        out.append(dict(what=f"{label} {what}", state=x.read_state(), logs=x.read_log(), digest=x.digest(), **more))

    groups, targets = parity_messages(x.R, x.G)
    snap("warm-up", counters=x.step(40))
    tickets = x.transfer(groups, targets)
    snap("transfer", tickets=tickets)
    snap("settle", counters=x.step(3))
    snap("resolve", states=x.resolve_transfers(groups, tickets))
    snap("evacuate", info=x.evacuate(np.full(max(x.G - 5, 0), EVACUATE_MASK, np.uint8), g0=3))
    snap("run-on", counters=x.step(40))
    return out


@functools.lru_cache(maxsize=None)
def host_parity_run(R: int, G: int, variant: str, g0: int = 0):
    """parity_run on the oracle, once per input and shared: (checkpoints, every
    counter row).  Treat it as read-only."""
    kw = RM.parity_kw(R, G, variant)
    h = Host(**kw, **({"g0": g0} if g0 else {}))
    points = parity_run(h, f"R{R} G{G} {variant}")
    h.close()
    return points, np.concatenate([p["counters"] for p in points if "counters" in p])


def assert_same_points(got: list, want: list, R: int):
    """Every checkpoint of the engine's parity_run equals the oracle's, bit for
    bit, as long as the run is valid: on a ring, up to the first step in which
    the oracle counts a window miss (restart_model.valid_rows)."""
    from helpers import assert_same_logs, assert_same_state
    assert len(got) == len(want)
    for a, b in zip(got, want):
        label = b["what"]
        if "counters" in b and not RM.assert_same_rows(a["counters"], b["counters"], label):
            return
        for k in ("tickets", "states"):
            if k in b:
                assert np.array_equal(a[k], b[k]), f"{label}: {k} differ at {np.nonzero(a[k] != b[k])[0][:5]}: " \
                                                   f"{a[k][a[k] != b[k]][:3]} vs {b[k][a[k] != b[k]][:3]}"
        assert a.get("info") == b.get("info"), f"{label}: info {a.get('info')} vs {b.get('info')}"
        assert_same_state(a["state"], b["state"], R, label)
        assert_same_logs(a["state"], a["logs"], b["logs"], R, label)
        assert a["digest"] == b["digest"], f"{label}: digest differs with equal state and logs"


# ---- the drain scenario: a node vacated before a planned restart.  Commands at 10 % of the group-steps: a
# follower is "caught up" only between a command and its replication, so at STRESS_MIX's 50 % a turn finds a
# target in about a third of the groups and 5 turns leave some group behind (a rate is an input, not a tolerance)
DRAIN_KW = dict(R=5, G=64, seed=11, log_cap=300, mode=abi.MODE_TEXTBOOK, ae_max_entries=4, cmd_ppm=100_000)
DRAIN_WARMUP, DRAIN_REPLICA, DRAIN_TURNS, DRAIN_DOWN = 60, 0, 5, 6


def drain_scenario(x, service_cls, drain: bool) -> dict:
    """On `x` (a Host or a RaftEngine) under service_cls (RaftService): warm
    up, stop the commands' effect on the followers' lag by draining (or not),
    restart DRAIN_REPLICA everywhere with down_steps, and count the groups with
    a leader at every step of the downtime."""
    svc = service_cls(x)
    x.step(DRAIN_WARMUP)
    remaining = turns = None
    if drain:
        remaining = svc.drain_node(DRAIN_REPLICA, DRAIN_TURNS)
        turns = svc.last_drain["turns"]
    before = int(x.step(1)[0, abi.C_INDEX["groups_with_leader"]])
    x.restart(np.full(x.G, 1 << DRAIN_REPLICA, np.uint8), down_steps=DRAIN_DOWN)
    during = x.step(DRAIN_DOWN)[:, abi.C_INDEX["groups_with_leader"]].astype(int).tolist()
    return dict(remaining=remaining, turns=turns, before=before, during=during)
