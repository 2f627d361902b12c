"""Committed-entry delivery restated in plain Python over read_state / read_log
(include/raft_engine.h, raft_engine_drain_committed): the reference of
test_apply_cpu.py (over the oracle) and test_gpu_apply.py (against the engine's
kernels).  Nothing here calls the engine."""
from __future__ import annotations

import functools

import numpy as np

import oracle as O
from helpers import abi, fld

EWINDOW = abi.RAFT_EWINDOW


def records(rows) -> np.ndarray:
    """(group, replica, index, term, cmd) tuples as an abi.APPLIED_DTYPE array."""
    out = np.zeros(len(rows), dtype=abi.APPLIED_DTYPE)
    if rows:
        out[:] = rows
    return out


def drain(state, terms, cmds, applied, R, cap, W=0, g0=0, n=None, replica=-1, room=None, peek=False):
    """One drain of groups [g0, g0 + n) of a whole engine's `state` [G, words],
    `terms` / `cmds` [G, R, cap] and `applied` [G, R] (updated in place unless
    peek): (records, info).  room None: no limit."""
    n = state.shape[0] - g0 if n is None else n
    rows, lost, regressed, pending = [], 0, 0, 0
    for g in range(g0, g0 + n):
        for r in (range(R) if replica < 0 else (replica,)):
            hi = int(np.clip(min(fld(state, R, r, "commit")[g], fld(state, R, r, "last")[g]), 0, cap))
            lo = int(applied[g, r])
            if W:                                                   # the ring: entries below the window are gone
                wl = max(0, int(fld(state, R, r, "phys")[g]) - W)
                if wl > lo and hi > lo:
                    lost += min(wl, hi) - lo
                    lo = min(wl, hi)
            if hi < lo:                                             # lastApplied is monotone
                regressed += 1
                continue
            for i in range(lo, hi):
                if peek or (room is not None and len(rows) >= room):
                    pending += hi - i
                    break
                rows.append((g, r, i, int(terms[g, r, i]), int(cmds[g, r, i])))
                lo = i + 1
            if not peek:
                applied[g, r] = lo
    info = {"delivered": len(rows), "pending": pending, "lost": lost, "regressed": regressed,
            "status": EWINDOW if lost else abi.RAFT_OK}
    return records(rows), info


@functools.lru_cache(maxsize=None)
def _run(kw_items, steps, every):
    kw = dict(kw_items)
    o = O.Oracle(abi.make_params(**kw))
    R, G, cap, W = kw["R"], kw["G"], kw["log_cap"], kw.get("log_window", 0)
    applied = np.zeros((G, R), np.int64)
    drains = []
    for _ in range(0, steps, every):
        o.step(every, counters=False)
        st = o.read_state()
        t, c = o.read_log()
        rec, info = drain(st, t, c, applied, R, cap, W)
        drains.append((rec, info, applied.copy()))
    final = (o.read_state(), *o.read_log(), o.digest())
    o.close()
    return drains, final


def oracle_run(steps: int, every: int, **kw):
    """The oracle stepped `steps` steps and drained every `every`: a list of
    (records, info, lastApplied after the drain) and the final (state, terms,
    cmds, digest).  Computed once per input and shared: treat it as read-only."""
    return _run(tuple(sorted(kw.items())), steps, every)


def totals(drains) -> dict:
    return {k: sum(d[1][k] for d in drains) for k in ("delivered", "lost", "regressed")}


def streams(drains, G: int, R: int):
    """Per (group, replica): the (index, term, cmd) it delivered, in order."""
    s = {(g, r): [] for g in range(G) for r in range(R)}
    for rec, _, _ in drains:
        for g, r, i, t, c in rec.tolist():
            s[(g, r)].append((i, t, c))
    return s


def prefix_violations(drains, G: int, R: int) -> int:
    """Replicas whose stream is not a prefix of their group's longest."""
    s = streams(drains, G, R)
    bad = 0
    for g in range(G):
        ref = max((s[(g, r)] for r in range(R)), key=len)
        bad += sum(s[(g, r)] != ref[: len(s[(g, r)])] for r in range(R))
    return bad
