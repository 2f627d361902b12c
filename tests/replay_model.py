"""WAL replay restated in numpy over exported state and logs
(include/ext/raft_replay.h, raft_wal_replay*): the batch rules and the effect.
The reference of test_replay_cpu.py (over the oracle, fed by wal_model's poll)
and test_gpu_replay.py (against the engine's kernels).  The volatile part of
the effect is restart_model's restart with flags 0.  Nothing here calls the
engine."""
from __future__ import annotations

import functools

import numpy as np

import oracle as O
import restart_model as RM
import wal_model as M
from helpers import F, STRESS_MIX, abi, fld

HS, TR, EN = M.HS, M.TR, M.EN
INFO_KEYS = ("applied", "replicas", "hardstates", "truncates", "entries", "malformed")
NF = abi.NUM_FIELDS


def last_index(state, R, g, r, cap) -> int:
    """lastIndex of the target now, taken within 0..log_cap."""
    return min(max(int(state[g, r * NF + F["last"]]), 0), cap)


def malformed(rows, m, state, R, cap, W=0) -> bool:
    """Record m of the batch `rows` (tuples) against its neighbours and the
    target's state: the rule of the header, one record at a time."""
    G = state.shape[0]
    g, r, kind, index, term, _, aux = rows[m]
    if not (0 <= g < G and 0 <= r < R) or kind not in (HS, TR, EN):
        return True
    same, pk, pindex = False, -1, 0
    if m > 0:
        pg, pr, pk, pindex = rows[m - 1][:4]
        if (pg, pr) > (g, r):
            return True                                              # the order of the runs
        same = (pg, pr) == (g, r)
        if same and (pk > kind or (pk == kind and kind != EN)):
            return True                                              # HARDSTATE, TRUNCATE, ENTRY... inside a run
    if kind == HS:
        return term < 0 or not -1 <= aux <= R
    last = last_index(state, R, g, r, cap)
    if kind == TR:
        return not 0 <= index <= last
    if not 0 <= index < cap:
        return True
    if same and pk == EN:
        if index != pindex + 1:
            return True
    elif same and pk == TR:
        if index != pindex:
            return True
    elif (index < last) if W else (index != last):
        return True
    return bool(W) and m + W < len(rows) and tuple(rows[m + W][:2]) == (g, r)   # one ring slot twice


def replay(state, terms, cmds, rec, *, R, cap, W=0, seed, step, gid0=0, emin, emax, keep_volatile=False) -> dict:
    """Apply the batch `rec` (abi.WAL_RECORD_DTYPE) to a whole engine's `state`
    [G, words] and `terms` / `cmds` [G, R, cap], in place; returns the info.
    A batch with a malformed record changes nothing and says how many."""
    rows = np.asarray(rec).tolist()
    info = dict.fromkeys(INFO_KEYS, 0)
    bad = sum(malformed(rows, m, state, R, cap, W) for m in range(len(rows)))
    if bad:
        info["malformed"] = bad
        return info
    sel = np.zeros((state.shape[0], R), bool)
    for g, r, kind, index, term, cmd, aux in rows:
        sel[g, r] = True
        w = state[g]
        info[("hardstates", "truncates", "entries")[kind]] += 1
        if kind == HS:
            w[r * NF + F["term"]], w[r * NF + F["voted"]] = term, aux
        elif kind == TR:
            w[r * NF + F["last"]] = w[r * NF + F["phys"]] = index
        else:
            terms[g, r, index], cmds[g, r, index] = term, cmd
            w[r * NF + F["last"]] = w[r * NF + F["phys"]] = index + 1
    info["applied"], info["replicas"] = len(rows), int(sel.sum())
    if not keep_volatile:
        RM.restart(state, sel, R=R, seed=seed, step=step, gid0=gid0, emin=emin, emax=emax)
    return info


def replay_into(x, rec, state, terms, cmds, keep_volatile=False) -> dict:
    """replay with the parameters of `x` (an Oracle or a RaftEngine: its
    raft_params `p` and step_index) on the exported arrays."""
    return replay(state, terms, cmds, rec, R=x.R, cap=int(x.p.log_cap), W=int(x.p.log_window), seed=int(x.p.seed),
                  step=int(x.step_index), gid0=int(x.p.g0), emin=int(x.p.election_min_ms),
                  emax=int(x.p.election_max_ms), keep_volatile=keep_volatile)


def pieces(rec, size: int):
    """The pieces max_records = size cuts out of one poll's records (polls of
    little room concatenate to one poll: test_wal_cpu.py, test_gpu_wal.py)."""
    return [rec[k:k + size] for k in range(0, len(rec), size)]


def persistent_errors(state, terms, cmds, want_state, want_terms, want_cmds, R, cap, W=0) -> list:
    """The (group, replica) whose currentTerm, votedFor, lastIndex or log
    [0, lastIndex) -- on a ring, the retained window of it -- differ from the
    source's."""
    bad = []
    idx = np.arange(cap)[None, :]
    for r in range(R):
        last = np.clip(fld(want_state, R, r, "last"), 0, cap)
        lo = np.maximum(0, fld(want_state, R, r, "phys") - W) if W else np.zeros_like(last)
        m = (idx >= lo[:, None]) & (idx < last[:, None])
        ok = np.ones(len(last), bool)
        for name in ("term", "voted", "last"):
            ok &= fld(state, R, r, name) == fld(want_state, R, r, name)
        ok &= ~np.any(m & ((terms[:, r] != want_terms[:, r]) | (cmds[:, r] != want_cmds[:, r])), axis=1)
        bad += [(int(g), r) for g in np.flatnonzero(~ok)]
    return bad


# ---- the oracle run of test_replay_cpu.py: textbook mode, the stress mix, polled every 1-7 steps

G, CAP, STEPS, PIECE, CHECK_EVERY = 203, 300, 400, 7, 50


def textbook(R: int) -> dict:
    return dict(R=R, G=G, seed=11, log_cap=CAP, mode=abi.MODE_TEXTBOOK, ae_max_entries=4, **STRESS_MIX)


def poll_steps(steps: int, seed: int) -> list:
    """The steps after which the source is polled: 1 to 7 apart, and every
    multiple of CHECK_EVERY among them."""
    rng = np.random.default_rng(seed)
    at, t = [], 0
    while t < steps:
        t = min(t + int(rng.integers(1, 8)), (t // CHECK_EVERY + 1) * CHECK_EVERY, steps)
        at.append(t)
    return at


@functools.lru_cache(maxsize=None)
def twin_run(R: int):
    """The oracle stepped STEPS steps; after each of poll_steps the model's
    poll, cut into pieces of PIECE records, each replayed with the model into a
    twin that started as a fresh engine's export.  Returns (checks, totals):
    per multiple of CHECK_EVERY the replicas whose persistent state differs, and
    the infos' sums with the poll's.  Computed once per R; read-only."""
    kw = textbook(R)
    o = O.Oracle(abi.make_params(**kw))
    try:
        twin = o.read_state()
        tt, tc = (np.zeros_like(a) for a in o.read_log())
        cur = M.fresh(G, R)
        tot = dict.fromkeys(INFO_KEYS + ("polled", "pieces", "lost"), 0)
        checks, t = [], 0
        for at in poll_steps(STEPS, R):
            o.step(at - t, counters=False)
            t = at
            st, (lt, lc) = o.read_state(), o.read_log()
            rec, pinfo = M.poll(st, lt, lc, cur, R, CAP)
            tot["polled"] += len(rec)
            tot["lost"] += pinfo["lost"]
            for piece in pieces(rec, PIECE):
                info = replay_into(o, piece, twin, tt, tc)
                tot["pieces"] += 1
                for k in INFO_KEYS:
                    tot[k] += info[k]
            if t % CHECK_EVERY == 0:
                checks.append((t, persistent_errors(twin, tt, tc, st, lt, lc, R, CAP)))
        return checks, tot
    finally:
        o.close()


# ---- hand-written batches, one per rule (test_replay_cpu.py on the model, test_gpu_replay.py on the engine)

CRAFT_G, CRAFT_R, CRAFT_CAP, CRAFT_W = 6, 3, 16, 4


def crafted():
    """(state, terms, cmds): every replica of 6 groups of 3 is in term 8, voted
    for 1 and holds 8 entries (term j + 1, cmd 100 g + 10 r + j), 6 committed."""
    w = np.zeros((CRAFT_G, abi.group_words(CRAFT_R)), np.int32)
    t = np.zeros((CRAFT_G, CRAFT_R, CRAFT_CAP), np.int32)
    c = np.zeros((CRAFT_G, CRAFT_R, CRAFT_CAP), np.uint32)
    for r in range(CRAFT_R):
        for name, v in (("term", 8), ("voted", 1), ("last", 8), ("phys", 8), ("commit", 6)):
            w[:, r * NF + F[name]] = v
        for g in range(CRAFT_G):
            t[g, r, :8] = np.arange(1, 9)
            c[g, r, :8] = 100 * g + 10 * r + np.arange(8)
    return w, t, c


def good_batch(ring: bool = False) -> np.ndarray:
    """A well-formed batch over the crafted state that uses every kind: a vote
    alone, a rewritten suffix, a log cut short, entries appended."""
    rows = [(0, 1, HS, -1, 9, 0, 2),
            (1, 0, HS, -1, 9, 0, -1), (1, 0, TR, 6, 0, 0, 0), (1, 0, EN, 6, 9, 70, 0), (1, 0, EN, 7, 9, 71, 0),
            (1, 0, EN, 8, 9, 72, 0),
            (2, 2, TR, 3, 0, 0, 0),
            (4, 1, EN, 8, 8, 80, 0), (4, 1, EN, 9, 8, 81, 0),
            (5, 2, HS, -1, 8, 0, 3), (5, 2, EN, 8, 8, 90, 0)]
    if ring:
        rows.append((5, 2, EN, 9, 8, 91, 0))
    return M.records(rows)


def malformed_batches(ring: bool = False) -> dict:
    """name -> (records, malformed records in it): one batch per rule, over the
    crafted state (lastIndex 8 everywhere; ring: log_window 4)."""
    ok = (1, 1, HS, -1, 9, 0, 1)
    b = {
        "order of replicas": ([(2, 1, HS, -1, 9, 0, 1), (2, 0, HS, -1, 9, 0, 1)], 1),
        "order of groups": ([(3, 0, HS, -1, 9, 0, 1), (2, 2, HS, -1, 9, 0, 1)], 1),
        "hardstate after truncate": ([(1, 1, TR, 8, 0, 0, 0), ok], 1),
        "two hardstates": ([ok, ok], 1),
        "two truncates": ([(1, 1, TR, 8, 0, 0, 0), (1, 1, TR, 7, 0, 0, 0)], 1),
        "truncate after entry": ([(1, 1, EN, 8, 8, 5, 0), (1, 1, TR, 9, 0, 0, 0)], 1),
        "a run in two parts": ([ok, (1, 2, HS, -1, 9, 0, 1), (1, 1, TR, 8, 0, 0, 0)], 1),
        "group below the engine": ([(-1, 0, HS, -1, 9, 0, 1), ok], 1),
        "group above the engine": ([ok, (CRAFT_G, 0, HS, -1, 9, 0, 1)], 1),
        "replica below 0": ([(1, -1, HS, -1, 9, 0, 1)], 1),
        "replica at R": ([(1, CRAFT_R, HS, -1, 9, 0, 1)], 1),
        "unknown kind": ([ok, (1, 1, 3, 0, 0, 0, 0)], 1),
        "negative kind": ([(1, 1, -1, 0, 0, 0, 0)], 1),
        "hardstate term below 0": ([(1, 1, HS, -1, -1, 0, 1)], 1),
        "hardstate vote below -1": ([(1, 1, HS, -1, 9, 0, -2)], 1),
        "hardstate vote above R": ([(1, 1, HS, -1, 9, 0, CRAFT_R + 1)], 1),
        "truncate above lastIndex": ([ok, (1, 1, TR, 9, 0, 0, 0)], 1),
        "truncate below 0": ([(1, 1, TR, -1, 0, 0, 0)], 1),
        # (a ring accepts a first entry above lastIndex: three entries reach log_cap there)
        "entry at log_cap": ([(1, 1, EN, j, 9, j, 0) for j in range(CRAFT_CAP - 2, CRAFT_CAP + 1)] if ring else
                             [(1, 1, TR, 8, 0, 0, 0)] + [(1, 1, EN, j, 9, j, 0) for j in range(8, CRAFT_CAP + 1)], 1),
        "first entry below lastIndex": ([ok, (1, 1, EN, 7, 9, 5, 0)], 1),
        "entry after truncate not at keep": ([(1, 1, TR, 6, 0, 0, 0), (1, 1, EN, 7, 9, 5, 0)], 1),
        "entries not consecutive": ([(1, 1, EN, 8, 9, 5, 0), (1, 1, EN, 10, 9, 6, 0)], 1),
        "entry repeated": ([(1, 1, EN, 8, 9, 5, 0), (1, 1, EN, 8, 9, 6, 0)], 1),
        "several at once": ([(0, 0, TR, 9, 0, 0, 0), (0, 0, EN, 8, 9, 5, 0), (0, 3, HS, -1, 9, 0, 1),
                             (0, 1, HS, -1, -5, 0, 1)], 4),
    }
    if ring:
        # five entries of one replica: the first and the fifth share slot 8 & 3
        b["more than log_window entries"] = ([(1, 1, EN, j, 9, j, 0) for j in range(8, 13)], 1)
        if CRAFT_CAP > 8 + CRAFT_W + 2:
            b["more than log_window entries after a hardstate"] = (
                [ok] + [(1, 1, EN, j, 9, j, 0) for j in range(8, 14)] + [(1, 2, HS, -1, 9, 0, 1)], 2)
    else:
        b["first entry above lastIndex"] = ([ok, (1, 1, EN, 9, 9, 5, 0)], 1)
    return {k: (M.records(rows), n) for k, (rows, n) in b.items()}
