"""The client path restated in plain Python over read_state / read_log arrays
and Oracle.append_command (include/raft_engine.h, raft_engine_read_leaders,
raft_propose_batch, raft_engine_resolve_tickets): the reference of
test_client_cpu.py (over the oracle alone) and test_gpu_client.py (against the
engine's kernels).  Nothing here calls the engine."""
from __future__ import annotations

import functools

import numpy as np

import oracle as O
from helpers import STRESS_MIX, abi, fld

ACCEPTED, GHOSTED, NO_LEADER, LOG_FULL = (abi.PROPOSE_ACCEPTED, abi.PROPOSE_GHOSTED, abi.PROPOSE_NO_LEADER,
                                          abi.PROPOSE_LOG_FULL)
NONE, COMMITTED, PENDING, LOST, UNKNOWN, INVALID = (abi.TICKET_NONE, abi.TICKET_COMMITTED, abi.TICKET_PENDING,
                                                    abi.TICKET_LOST, abi.TICKET_UNKNOWN, abi.TICKET_INVALID)


def leaders(state: np.ndarray, R: int) -> np.ndarray:
    """The leader directory of every group of `state` [G, words]."""
    out = np.zeros(state.shape[0], dtype=abi.LEADER_DTYPE)
    out["leader"] = -1
    for r in reversed(range(R)):                                   # descending: the lowest id is taken last
        lead = fld(state, R, r, "role") == abi.LEADER
        out["n_leaders"] += lead
        out["leader"][lead] = r
        out["term"][lead] = fld(state, R, r, "term")[lead]
        out["commit"][lead] = fld(state, R, r, "commit")[lead]
    return out


def propose(o: O.Oracle, groups, cmds, textbook: bool = False, W: int = 0):
    """One propose batch on the oracle: the leaders are looked up in the state
    the call finds, the messages applied in batch order with
    Oracle.append_command; (tickets, return code).  The tickets' indices and
    statuses come from lastIndex / physLen tracked here by the rules of the
    header; the oracle's own state afterwards must agree with them."""
    groups = np.asarray(groups, dtype=np.int64)
    if len(groups) and (groups.min() < 0 or groups.max() >= o.G):
        return None, abi.RAFT_ERANGE                               # nothing is applied
    st = o.read_state()
    R, cap = o.R, o.cap
    ld = leaders(st, R)
    tickets = np.zeros(len(groups), dtype=abi.TICKET_DTYPE)
    cur = {}                                                       # group -> [lastIndex, physLen] of its leader
    miss = 0
    for m, (g, c) in enumerate(zip(groups.tolist(), np.asarray(cmds).tolist())):
        r = int(ld["leader"][g])
        if r < 0:
            tickets[m] = (-1, -1, 0, NO_LEADER)
            continue
        lp = cur.setdefault(g, [int(fld(st, R, r, "last")[g]), int(fld(st, R, r, "phys")[g])])
        last, phys = lp
        if textbook:                                               # an array log: slot lastIndex is written
            status = LOG_FULL if last >= cap else ACCEPTED
            if status == ACCEPTED:
                miss += bool(W) and last < phys - W
                lp[:] = [last + 1, max(phys, last + 1)]
        else:                                                      # Commons.kt:58-61: appended at the physical end (Q1)
            status = LOG_FULL if phys >= cap else GHOSTED if phys != last else ACCEPTED
            if status != LOG_FULL:
                lp[:] = [last + 1, phys + 1]
        tickets[m] = (r, last, int(ld["term"][g]), status)
        o.append_command(g, r, c)
    after = o.read_state()
    for g, (last, phys) in cur.items():
        r = int(ld["leader"][g])
        assert (fld(after, R, r, "last")[g], fld(after, R, r, "phys")[g]) == (last, phys), (g, r, last, phys)
    return tickets, (abi.RAFT_EWINDOW if miss else abi.RAFT_OK)


def resolve(state, terms, logcmds, groups, tickets, cmds, R: int, cap: int, W: int = 0):
    """raft_engine_resolve_tickets over a whole engine's `state` [G, words] and
    `terms` / `logcmds` [G, R, cap]: (records, return code)."""
    groups = np.asarray(groups, dtype=np.int64)
    cmds = np.asarray(cmds, dtype=np.uint32)
    n, G = len(groups), state.shape[0]
    out = np.zeros(n, dtype=abi.TICKET_STATE_DTYPE)
    g_ok = (groups >= 0) & (groups < G)
    stored = (tickets["status"] != NO_LEADER) & (tickets["status"] != LOG_FULL)
    t_ok = (tickets["replica"] >= -1) & (tickets["replica"] < R) & (tickets["index"] >= 0) & (tickets["index"] < cap)
    look = g_ok & stored & t_ok
    g = np.where(look, groups, 0)
    i = np.where(look, tickets["index"], 0).astype(np.int64)
    holders, com, unk, own = (np.zeros(n, np.int32) for _ in range(4))
    for r in range(R):
        last, phys, commit = (fld(state, R, r, f)[g].astype(np.int64) for f in ("last", "phys", "commit"))
        below = look & (i < phys - W) if W else np.zeros(n, bool)
        same = (terms[g, r, i] == tickets["term"]) & (logcmds[g, r, i] == cmds)
        hold = look & ~below & (i < last) & same
        hi = np.clip(np.minimum(commit, last), 0, cap)
        holders += hold
        com += hold & (i < hi)
        unk += below
        own += hold & (tickets["replica"] == r)
    status = np.where(com >= 1, COMMITTED, np.where(unk >= 1, UNKNOWN, np.where(own >= 1, PENDING, LOST)))
    status = np.where(~g_ok, INVALID, np.where(~stored, NONE, np.where(~t_ok, INVALID, status)))
    out["status"], out["holders"], out["committed_on"], out["unknown"] = status, holders, com, unk
    rc = (abi.RAFT_ERANGE if (~g_ok).any() else abi.RAFT_EINVAL if (g_ok & stored & ~t_ok).any()
          else abi.RAFT_EWINDOW if (status == UNKNOWN).any() else abi.RAFT_OK)
    return out, rc


# ---- the lockstep run: the oracle stepped and proposed to, every ticket resolved ----
SIZES = (1, 63, 64, 65, 700)           # batch sizes, cycled; the largest carries the hot group's burst
# the harness's own commands off (cmd_ppm 0): every command is a proposal.  A
# log_window run must stay free of window misses to be comparable at all (a
# miss is served differently by a ring and by the oracle's full lists), so the
# ring runs take message drops alone, as the drain's ring runs do
FLAT_MIX = dict(STRESS_MIX, cmd_ppm=0)
RING_MIX = dict(drop_ppm=50_000, cmd_ppm=0)


def hot_burst(W: int) -> int:
    """Messages the hot group gets out of a batch of 700: 70 (more than a
    wave) on a flat log.  In a W-slot ring a leader that runs 70 entries ahead
    makes its followers' catch-up read below its window (physLen - W), which
    invalidates the run by the window's own rule (RAFT_C_LOG_WINDOW_MISS): there
    the burst is W / 2."""
    return W // 2 if W else 70


def batch_of(rng, size: int, G: int, k: int, W: int):
    """Batch k: uniformly random groups; a batch of 700 interleaves the hot
    group's burst among the others.  The hot group moves with k, so no group
    comes near log_cap over the run."""
    groups = rng.integers(0, G, size, dtype=np.int64)
    if size == 700:
        groups[rng.choice(size, hot_burst(W), replace=False)] = (37 * k + 11) % G
    return groups, rng.integers(1, 2 ** 32, size, dtype=np.uint32)


@functools.lru_cache(maxsize=None)
def _run(kw_items, steps, every, batch_seed):
    kw = dict(kw_items)
    o = O.Oracle(abi.make_params(**kw))
    R, G, cap, W, tb = kw["R"], kw["G"], kw["log_cap"], kw.get("log_window", 0), kw.get("mode", 0) == 1
    rng = np.random.default_rng(batch_seed)
    all_g, all_t, all_c = (np.zeros(0, np.int64), np.zeros(0, abi.TICKET_DTYPE), np.zeros(0, np.uint32))
    batches, rows = [], []
    for k in range(steps // every):
        rows.append(o.step(every))
        groups, cmds = batch_of(rng, SIZES[k % len(SIZES)], G, k, W)
        before = leaders(o.read_state(), R)
        tickets, prc = propose(o, groups, cmds, tb, W)
        all_g, all_t, all_c = np.concatenate([all_g, groups]), np.concatenate([all_t, tickets]), np.concatenate([all_c, cmds])
        rec, rrc = resolve(o.read_state(), *o.read_log(), all_g, all_t, all_c, R, cap, W)
        batches.append(dict(groups=groups, cmds=cmds, leaders=before, tickets=tickets, propose_rc=prc,
                            records=rec, resolve_rc=rrc, digest=o.digest()))
    rows.append(o.step(every))                                     # the steps after the last batch
    counters = np.concatenate(rows)
    final = (o.read_state(), *o.read_log(), o.digest())
    o.close()
    tot = {n: int(counters[:, i].sum()) for n, i in abi.C_INDEX.items()}
    # conditions on the inputs: leaders were elected, entries committed, nothing overflowed, no window miss
    assert tot["leaders_elected"] > 0 and tot["commits"] > 0 and tot["commands"] == 0, tot
    assert tot["log_overflow"] == 0 and tot["log_window_miss"] == 0, tot
    return batches, counters, (all_g, all_t, all_c), final


def oracle_run(steps: int, every: int, batch_seed: int = 5, **kw):
    """The oracle stepped `steps` steps; after every `every` a batch of
    batch_of() (drawn from `batch_seed`) is proposed and every ticket issued so far resolved.  Returns
    (batches, counters [steps + every, stride], (groups, tickets, cmds) of every
    ticket, final (state, terms, cmds, digest)).  batches[k]: groups, cmds,
    leaders (the directory the batch found), tickets, propose_rc, records (of
    every ticket so far), resolve_rc, digest (after the batch).  Computed once
    per input and shared: treat it as read-only."""
    return _run(tuple(sorted(kw.items())), steps, every, batch_seed)


def history(batches) -> np.ndarray:
    """[tickets, batches] resolve statuses of each ticket, -1 before it was issued."""
    n = len(batches[-1]["records"])
    h = np.full((n, len(batches)), -1, np.int32)
    for k, b in enumerate(batches):
        h[: len(b["records"]), k] = b["records"]["status"]
    return h


# ---- a crafted engine: every routing and Log.add situation in eight groups ----
def crafted(R: int = 3, G: int = 8, cap: int = 16):
    """(state, terms, cmds) of 8 groups of 3 replicas, every replica holding 5
    entries (term 1 + j // 2, cmd 1000 g + 100 r + j), 3 of them committed:
      0 no leader            1 one leader (replica 1)    2 two leaders (0 and 2: 0 wins)
      3 a leader at R - 1    4 a leader with physLen 7 > lastIndex 5 (a ghost tail)
      5 a leader whose log is full (lastIndex = physLen = log_cap)
      6 a leader all replicas agree with (its committed entries resolve COMMITTED)
      7 candidates only"""
    from helpers import blank_groups, set_fld
    assert (R, G) == (3, 8)
    w = blank_groups(G, R)
    t = np.zeros((G, R, cap), np.int32)
    c = np.zeros((G, R, cap), np.uint32)
    for g in range(G):
        for r in range(R):
            t[g, r] = 1 + np.arange(cap) // 2
            c[g, r] = 1000 * g + 100 * r + np.arange(cap)
    c[6, :] = c[6, 0]                                              # group 6: identical logs
    for r in range(R):
        set_fld(w, R, r, "term", 4)
        set_fld(w, R, r, "last", 5)
        set_fld(w, R, r, "phys", 5)
        set_fld(w, R, r, "commit", 3)
    for g, r in ((1, 1), (2, 0), (2, 2), (3, R - 1), (4, 0), (5, 0), (6, 1)):
        set_fld(w[g:g + 1], R, r, "role", abi.LEADER)
    set_fld(w[2:3], R, 0, "term", 5)                               # the two leaders differ in term and commit
    set_fld(w[2:3], R, 0, "commit", 2)
    set_fld(w[4:5], R, 0, "phys", 7)
    set_fld(w[5:6], R, 0, "last", cap)
    set_fld(w[5:6], R, 0, "phys", cap)
    for r in range(R):
        set_fld(w[7:8], R, r, "role", abi.CANDIDATE)
    return w, t, c


# one batch on the crafted engine: three proposals to group 1 interleaved among the others, two to the ghost tail
CRAFTED_GROUPS = np.array([1, 0, 2, 1, 3, 4, 5, 1, 6, 7, 4, 5], dtype=np.int64)
CRAFTED_CMDS = np.arange(9001, 9001 + len(CRAFTED_GROUPS), dtype=np.uint32)


def crafted_oracle(textbook: bool, R: int = 3, G: int = 8, cap: int = 16):
    kw = dict(R=R, G=G, log_cap=cap, **(dict(mode=1) if textbook else {}))
    o = O.Oracle(abi.make_params(**kw))
    w, t, c = crafted(R, G, cap)
    o.write_state(w)
    o.write_log(t, c)
    assert np.array_equal(o.read_state(), w)
    return o, kw
