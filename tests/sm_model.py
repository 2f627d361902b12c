"""The replicated state machine restated in plain Python over read_state /
read_log (include/raft_engine.h, raft_engine_sm_*): the reference of
test_sm_cpu.py (over the oracle) and test_gpu_sm.py (against the engine's
kernels).  Python ints masked to 64 bits; nothing here calls the engine."""
from __future__ import annotations

import functools

import numpy as np

import apply_model as A
import oracle as O
from helpers import abi, fld

MASK = (1 << 64) - 1
P = 0xD1342543DE82EF95
GOLD = 0x9E3779B97F4A7C15
EWINDOW = abi.RAFT_EWINDOW


def fmix(z: int) -> int:
    z ^= z >> 30
    z = z * 0xBF58476D1CE4E5B9 & MASK
    z ^= z >> 27
    z = z * 0x94D049BB133111EB & MASK
    return z ^ z >> 31


def x_of(i: int, t: int, c: int) -> int:
    return fmix(((((t & 0xFFFFFFFF) << 32) | (c & 0xFFFFFFFF)) + (i & 0xFFFFFFFF) * GOLD) & MASK)


def fold(xs, h: int = 0) -> int:
    """The sequential hash of the values xs on top of h."""
    for x in xs:
        h = (h * P + x) & MASK
    return h


class Machine:
    """Every replica's machine of G groups: reg [G, R, S], hash, applied, lost [G, R]."""

    def __init__(self, G: int, R: int, S: int):
        self.G, self.R, self.S = G, R, S
        self.reg = np.zeros((G, R, S), np.uint32)
        self.hash = np.zeros((G, R), np.uint64)
        self.applied = np.zeros((G, R), np.int64)
        self.lost = np.zeros((G, R), np.int64)

    def apply_entry(self, g: int, r: int, i: int, t: int, c: int):
        """The per-entry rule: last writer wins in the slot, the hash folds x(i, t, c)."""
        self.reg[g, r, c & (self.S - 1)] = c
        self.hash[g, r] = (int(self.hash[g, r]) * P + x_of(i, t, c)) & MASK

    def heads(self, g0: int = 0, n: int | None = None) -> np.ndarray:
        n = self.G - g0 if n is None else n
        h = np.zeros((n, self.R), abi.SM_HEAD_DTYPE)
        h["applied"], h["lost"], h["hash"] = self.applied[g0:g0 + n], self.lost[g0:g0 + n], self.hash[g0:g0 + n]
        return h

    def copy(self) -> "Machine":
        m = Machine(self.G, self.R, self.S)
        m.reg, m.hash, m.applied, m.lost = self.reg.copy(), self.hash.copy(), self.applied.copy(), self.lost.copy()
        return m


def apply(state, terms, cmds, mach: Machine, R, cap, W=0, g0=0, n=None, replica=-1) -> dict:
    """One sm_apply of groups [g0, g0 + n) of a whole engine's `state` [G, words]
    and `terms` / `cmds` [G, R, cap] into `mach` (in place): the info."""
    n = state.shape[0] - g0 if n is None else n
    applied = lost = regressed = 0
    col = lambda name: np.stack([fld(state, R, r, name) for r in range(R)], -1).astype(np.int64)     # [G, R]
    his = np.clip(np.minimum(col("commit"), col("last")), 0, cap).tolist()
    phys = col("phys").tolist()
    for g in range(g0, g0 + n):
        for r in (range(R) if replica < 0 else (replica,)):
            hi = his[g][r]
            lo = int(mach.applied[g, r])
            if W:                                                   # the ring: entries below the window are gone
                wl = max(0, phys[g][r] - W)
                if wl > lo and hi > lo:
                    skip = min(wl, hi) - lo
                    lost += skip
                    mach.lost[g, r] += skip
                    lo += skip
                    mach.applied[g, r] = lo
            if hi < lo:                                             # the cursor is monotone
                regressed += 1
                continue
            h, reg, mask = int(mach.hash[g, r]), mach.reg[g, r], mach.S - 1
            for i, t, c in zip(range(lo, hi), terms[g, r, lo:hi].tolist(), cmds[g, r, lo:hi].tolist()):
                reg[c & mask] = c                                   # apply_entry, on Python ints
                h = (h * P + x_of(i, t, c)) & MASK
            mach.hash[g, r] = h
            applied += hi - lo
            mach.applied[g, r] = hi
    return {"applied": applied, "lost": lost, "regressed": regressed, "status": EWINDOW if lost else abi.RAFT_OK}


def leader_of(state, R, g) -> int:
    """raft_leader_info.leader: the lowest replica index whose role is LEADER, or -1."""
    return next((r for r in range(R) if fld(state, R, r, "role")[g] == abi.LEADER), -1)


def get(state, mach: Machine, R, groups, keys, replicas) -> np.ndarray:
    out = np.zeros(len(groups), abi.SM_VALUE_DTYPE)
    for m, (g, k, r) in enumerate(zip(groups, keys, replicas)):
        r = leader_of(state, R, g) if r < 0 else r
        out[m] = (0, -1, 0, 0) if r < 0 else (mach.reg[g, r, k & (mach.S - 1)], r, mach.applied[g, r],
                                               fld(state, R, r, "commit")[g])
    return out


def check(mach: Machine) -> np.ndarray:
    """Per group: 1 if two replicas have lost == 0, equal applied and different hash."""
    f = np.zeros(mach.G, np.uint8)
    for g in range(mach.G):
        for a in range(mach.R):
            for b in range(a + 1, mach.R):
                if mach.lost[g, a] == 0 and mach.lost[g, b] == 0 and mach.applied[g, a] == mach.applied[g, b] \
                        and mach.hash[g, a] != mach.hash[g, b]:
                    f[g] = 1
    return f


@functools.lru_cache(maxsize=None)
def _run(kw_items, steps, every, slots, drain_every):
    kw = dict(kw_items)
    o = O.Oracle(abi.make_params(**kw))
    R, G, cap, W = kw["R"], kw["G"], kw["log_cap"], kw.get("log_window", 0)
    mach = Machine(G, R, slots)
    drained = np.zeros((G, R), np.int64)
    points = []
    for k in range(steps // every):
        o.step(every, counters=False)
        st = o.read_state()
        t, c = o.read_log()
        info = apply(st, t, c, mach, R, cap, W)
        d = A.drain(st, t, c, drained, R, cap, W) if drain_every and (k + 1) % drain_every == 0 else None
        points.append((info, mach.heads(), mach.reg.copy(), d))
    final = (o.read_state(), *o.read_log(), o.digest())
    o.close()
    return points, final, mach


def oracle_run(steps: int, every: int, slots: int, drain_every: int = 0, **kw):
    """The oracle stepped `steps` steps with the model applied every `every`: a
    list of (info, heads, regs, drain) per apply -- drain the (records, info) of
    an apply_model.drain of everything taken right after every `drain_every`-th
    apply, else None -- then the final (state, terms, cmds, digest) and the
    final Machine.  Computed once per input and shared: treat it as read-only."""
    return _run(tuple(sorted(kw.items())), steps, every, slots, drain_every)
