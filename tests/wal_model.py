"""The persistence stream restated in plain Python over read_state / read_log
and a cursor array (include/raft_engine.h, raft_wal_poll): the reference of
test_wal_cpu.py (over the oracle) and test_gpu_wal.py (against the engine's
kernels), and an image-applier of its own, so that neither leans on the
package's WalImage.  Nothing here calls the engine."""
from __future__ import annotations

import functools

import numpy as np

import oracle as O
from helpers import abi, fld

EWINDOW = abi.RAFT_EWINDOW
HS, TR, EN = abi.WAL_HARDSTATE, abi.WAL_TRUNCATE, abi.WAL_ENTRY
INFO_KEYS = ("delivered", "pending", "hardstates", "truncates", "entries", "lost", "regressed")


def records(rows) -> np.ndarray:
    """(group, replica, kind, index, term, cmd, aux) tuples as an abi.WAL_RECORD_DTYPE array."""
    out = np.zeros(len(rows), dtype=abi.WAL_RECORD_DTYPE)
    if rows:
        out[:] = rows
    return out


def fresh(G: int, R: int) -> np.ndarray:
    """The cursors of a new handle: [G, R] of abi.WAL_CURSOR_DTYPE."""
    cur = np.zeros((G, R), dtype=abi.WAL_CURSOR_DTYPE)
    cur["vote"] = -1
    return cur


def poll(state, terms, cmds, cur, R, cap, W=0, g0=0, n=None, replica=-1, room=None, peek=False, stats=None):
    """One poll of groups [g0, g0 + n) of a whole engine's `state` [G, words],
    `terms` / `cmds` [G, R, cap] and the cursors `cur` [G, R] (updated in place
    unless peek): (records, info).  room None: no limit.  stats (a dict) counts
    what the coverage conditions ask for: TRUNCATEs below stable, replicas
    re-sent from a floor above 0, replicas with a HARDSTATE and a TRUNCATE."""
    n = state.shape[0] - g0 if n is None else n
    rs = list(range(R)) if replica < 0 else [replica]
    f = {k: {r: fld(state, R, r, k)[g0:g0 + n].tolist() for r in rs} for k in ("term", "voted", "last", "phys", "commit")}
    rows, total, lost, regressed = [], 0, 0, 0
    kinds = [0, 0, 0]
    for j in range(n):
        g = g0 + j
        for r in rs:
            term, voted, last_raw, phys, commit = (f[k][r][j] for k in ("term", "voted", "last", "phys", "commit"))
            last = min(max(last_raw, 0), cap)
            hi = min(max(min(commit, last_raw), 0), cap)
            wl = max(0, phys - W) if W else 0
            c_term, c_vote, stable, sterm, floor, _ = cur[g, r].tolist()
            run = []
            if (term, voted) != (c_term, c_vote):
                run.append((g, r, HS, -1, term, 0, voted))
            clean = stable <= last and (stable == 0 or (stable - 1 >= wl and int(terms[g, r, stable - 1]) == sterm))
            frm = stable
            if not clean:
                keep = min(floor, last)
                regressed += keep < floor
                run.append((g, r, TR, keep, 0, 0, 0))
                frm = keep
                if stats is not None:
                    stats["below_stable"] = stats.get("below_stable", 0) + (keep < stable)
                    stats["from_floor"] = stats.get("from_floor", 0) + (keep == floor > 0)
                    stats["hs_and_tr"] = stats.get("hs_and_tr", 0) + (len(run) == 2)
            first = max(frm, min(wl, last))
            lost += first - frm
            if last > first:
                run += zip([g] * (last - first), [r] * (last - first), [EN] * (last - first), range(first, last),
                           terms[g, r, first:last].tolist(), cmds[g, r, first:last].tolist(), [0] * (last - first))
            total += len(run)
            if peek:
                continue
            wrote = run if room is None else run[: max(0, room - len(rows))]
            truncated = False
            for _, _, kind, index, t, _, aux in wrote:
                kinds[kind] += 1
                if kind == HS:
                    c_term, c_vote = t, aux
                elif kind == TR:
                    truncated = True
                    stable = index
                    sterm = int(terms[g, r, index - 1]) if index > 0 and index - 1 >= wl else 0
                else:
                    stable, sterm = index + 1, t
            if clean or truncated:                                  # the handed-out prefix is the replica's log
                floor = min(hi, stable)
            cur[g, r] = (c_term, c_vote, stable, sterm, floor, 0)
            rows += wrote
    info = {"delivered": len(rows), "pending": total - len(rows), "hardstates": kinds[HS], "truncates": kinds[TR],
            "entries": kinds[EN], "lost": lost, "regressed": int(regressed), "status": EWINDOW if lost else abi.RAFT_OK}
    return records(rows), info


class Image:
    """The ten-line applier: what the records build, per (group, replica)."""

    def __init__(self, G, R, cap, gaps=False):
        self.term, self.vote = np.zeros((G, R), np.int64), np.full((G, R), -1, np.int64)
        self.length, self.gaps = np.zeros((G, R), np.int64), gaps
        self.terms, self.cmds = np.zeros((G, R, cap), np.int64), np.zeros((G, R, cap), np.int64)

    def apply(self, rec):
        for g, r, kind, index, term, cmd, aux in rec.tolist():
            if kind == HS:
                self.term[g, r], self.vote[g, r] = term, aux
            elif kind == TR:
                assert 0 <= index <= self.length[g, r], ("TRUNCATE above the length", g, r, index)
                self.length[g, r] = index
            else:
                assert index == self.length[g, r] or (self.gaps and index > self.length[g, r]), ("ENTRY", g, r, index)
                self.terms[g, r, index], self.cmds[g, r, index], self.length[g, r] = term, cmd, index + 1

    def errors(self, state, terms, cmds, R, cap, W=0) -> list:
        """Where the image differs from the replicas' term, vote and log
        [0, lastIndex) -- on a ring, from the retained window of it."""
        bad = []
        idx = np.arange(cap)[None, :]
        for r in range(R):
            last = np.clip(fld(state, R, r, "last"), 0, cap)
            lo = np.maximum(0, fld(state, R, r, "phys") - W) if W else np.zeros_like(last)
            m = (idx >= lo[:, None]) & (idx < last[:, None])
            ok = (self.term[:, r] == fld(state, R, r, "term")) & (self.vote[:, r] == fld(state, R, r, "voted")) & \
                (self.length[:, r] == last) & ~np.any(m & ((self.terms[:, r] != terms[:, r]) |
                                                           (self.cmds[:, r] != cmds[:, r])), axis=1)
            bad += [(int(g), r) for g in np.flatnonzero(~ok)]
        return bad


@functools.lru_cache(maxsize=None)
def _run(kw_items, steps, every):
    kw = dict(kw_items)
    o = O.Oracle(abi.make_params(**kw))
    R, G, cap, W = kw["R"], kw["G"], kw["log_cap"], kw.get("log_window", 0)
    cur, img, stats = fresh(G, R), Image(G, R, cap, gaps=W > 0), {}
    polls, image_errors = [], []
    for _ in range(0, steps, every):
        o.step(every, counters=False)
        st = o.read_state()
        t, c = o.read_log()
        rec, info = poll(st, t, c, cur, R, cap, W, stats=stats)
        img.apply(rec)
        image_errors.append(img.errors(st, t, c, R, cap, W))
        polls.append((rec, info, cur.copy()))
    final = (o.read_state(), *o.read_log(), o.digest())
    o.close()
    return polls, final, image_errors, stats


def oracle_run(steps: int, every: int, **kw):
    """The oracle stepped `steps` steps and polled every `every`: a list of
    (records, info, cursors after the poll), the final (state, terms, cmds,
    digest), per poll the replicas whose applied image differs from the
    oracle, and the coverage counts.  Computed once per input and shared:
    treat it as read-only."""
    return _run(tuple(sorted(kw.items())), steps, every)


def totals(polls) -> dict:
    return {k: sum(p[1][k] for p in polls) for k in INFO_KEYS}
