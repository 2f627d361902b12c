"""Replica restart restated in numpy over the canonical state words
(include/raft_engine.h, raft_engine_restart*): the reference of
test_restart_cpu.py (over the oracle) and test_gpu_restart.py (against the
engine's kernel).  The draws come from the engine's host-side Philox; nothing
here touches a device."""
from __future__ import annotations

import functools
import importlib

import numpy as np

import apply_model as A
import oracle as O
import sm_model as M
from helpers import F, STRESS_MIX, abi, assert_same_logs, assert_same_state, fld

philox4x32_10 = importlib.import_module("raft-kotlin_amd.engine").philox4x32_10

AMNESIA, REPLAY = abi.RESTART_AMNESIA, abi.RESTART_REPLAY


def ppm_thr(ppm: int, bits: int = 32) -> int:
    """ceil(ppm * 2^bits / 10^6): w hits when w < ppm_thr."""
    return -(-(ppm << bits) // 1_000_000)


def scale_range(w: int, lo: int, hi: int) -> int:
    """(lo..hi).random() from a 32-bit word by multiply-shift (philox.h scale_range)."""
    return lo + ((w * (((hi - lo) & 0xFFFFFFFF) + 1 & 0xFFFFFFFF)) >> 32)


def key_of(seed: int):
    return [seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF]


def rng_word(seed: int, step: int, gid: int, purpose: int, r: int) -> int:
    """Word r & 3 of philox(c0 = step mod 2^32, c1 = gid, c2 = purpose, c3 = r >> 2)."""
    return philox4x32_10([step & 0xFFFFFFFF, gid & 0xFFFFFFFF, purpose, r >> 2], key_of(seed))[r & 3]


def select_mask(mask, R: int) -> np.ndarray:
    """[n, R] bool from n mask bytes; bits at or above R are ignored."""
    m = np.asarray(mask, dtype=np.uint8)
    return ((m[:, None] >> np.arange(R, dtype=np.uint8)[None, :]) & 1).astype(bool)


def select_random(seed: int, step: int, gid0: int, n: int, R: int, ppm: int) -> np.ndarray:
    """[n, R] bool: the seeded selection of global group ids gid0 .. gid0 + n - 1."""
    thr = ppm_thr(ppm, 32)
    sel = np.zeros((n, R), dtype=bool)
    for j in range(n):
        for r in range(R):
            sel[j, r] = rng_word(seed, step, gid0 + j, abi.RNG_RESTART, r) < thr
    return sel


def mask_of(sel: np.ndarray) -> np.ndarray:
    return (sel.astype(np.uint8) << np.arange(sel.shape[1], dtype=np.uint8)[None, :]).sum(axis=1).astype(np.uint8)


def restart(state: np.ndarray, sel: np.ndarray, *, R: int, seed: int, step: int, gid0: int, emin: int, emax: int,
            flags: int = 0, down_steps: int = 0, applied=None, heads=None, regs=None) -> dict:
    """Restart the replicas sel [n, R] of the n groups in `state` [n, words]
    (global ids gid0 ..), in place; applied [n, R], heads [n, R] of
    abi.SM_HEAD_DTYPE and regs [n, R, S] are those groups' consumers (None:
    absent).  Returns the info."""
    n = state.shape[0]
    assert sel.shape == (n, R)
    info = {"restarted": 0, "leaders": 0, "entries_dropped": 0}
    NF = abi.NUM_FIELDS
    for j in range(n):
        rs = [r for r in range(R) if sel[j, r]]
        for r in rs:
            w = state[j]
            info["restarted"] += 1
            info["leaders"] += int(w[r * NF + F["role"]] == abi.LEADER)
            w[r * NF + F["role"]] = abi.FOLLOWER
            w[r * NF + F["commit"]] = 0
            w[r * NF + F["phase_ms"]] = 0
            w[r * NF + F["retry_ms"]] = 0
            w[r * NF + F["flags"]] = abi.FL_ARMED
            w[r * NF + F["election_ms"]] = scale_range(rng_word(seed, step, gid0 + j, abi.RNG_TIMER, r), emin, emax)
            w[R * NF + r * R:R * NF + (r + 1) * R] = 0                       # next[r][*]
            w[R * NF + R * R + r * R:R * NF + R * R + (r + 1) * R] = 0       # match[r][*]
            if flags & AMNESIA:
                info["entries_dropped"] += int(w[r * NF + F["last"]])
                w[r * NF + F["term"]] = 0
                w[r * NF + F["voted"]] = -1
                w[r * NF + F["last"]] = 0
                w[r * NF + F["phys"]] = 0
            if flags & (AMNESIA | REPLAY):
                if applied is not None:
                    applied[j, r] = 0
                if heads is not None:
                    heads[j, r] = (0, 0, 0)
                if regs is not None:
                    regs[j, r] = 0
        if rs and down_steps > 0:
            state[j, -2] = (down_steps << 8) | rs[0]
    return info


def restart_engine_like(x, sel, *, g0: int, flags: int = 0, down_steps: int = 0, applied=None, heads=None,
                        regs=None) -> dict:
    """The host route on anything with read_state / write_state / step_index and
    raft_params `p` (the Oracle, or a RaftEngine): read -> model -> write of
    groups [g0, g0 + len(sel))."""
    n = sel.shape[0]
    st = x.read_state(g0, n)
    info = restart(st, sel, R=x.R, seed=int(x.p.seed), step=int(x.step_index), gid0=int(x.p.g0) + g0,
                   emin=int(x.p.election_min_ms), emax=int(x.p.election_max_ms), flags=flags, down_steps=down_steps,
                   applied=None if applied is None else applied[g0:g0 + n],
                   heads=None if heads is None else heads[g0:g0 + n], regs=None if regs is None else regs[g0:g0 + n])
    x.write_state(st, g0)
    return info


class Host:
    """The oracle with the consumers' models beside it (apply_model's drain
    cursor, sm_model's machine), under RaftEngine's method names: what the
    engine must equal when both are driven through the same calls.  restart is
    read_state -> restart() above -> write_state.  `hits` counts what the
    restarts met (the non-vacuity conditions of test_restart_cpu.py)."""

    def __init__(self, slots: int = 0, **kw):
        self.p = abi.make_params(**kw)
        self.o = O.Oracle(self.p)
        self.R, self.G, self.cap, self.W = kw["R"], kw["G"], kw["log_cap"], kw.get("log_window", 0)
        self.cursor = np.zeros((self.G, self.R), np.int64)
        self.mach = M.Machine(self.G, self.R, slots) if slots else None
        self.hits = {"leader": 0, "committed": 0, "two": 0, "all": 0, "restarted": 0, "spared": 0}

    def close(self):
        self.o.close()

    @property
    def step_index(self) -> int:
        return int(self.o.step_index)

    def step(self, n: int):
        return self.o.step(n)[:, : abi.NUM_COUNTERS]

    def read_state(self, g0=0, n=None):
        return self.o.read_state(g0, n)

    def read_log(self, g0=0, n=None):
        return self.o.read_log(g0, n)

    def digest(self) -> int:
        return self.o.digest()

    def applied(self):
        return self.cursor.astype(np.int32)

    def sm_read(self):
        return self.mach.heads(), self.mach.reg.copy()

    def drain_committed(self, g0=0, n=None, replica=-1):
        return A.drain(self.o.read_state(), *self.o.read_log(), self.cursor, self.R, self.cap, self.W, g0, n, replica)

    def sm_apply(self, g0=0, n=None, replica=-1) -> dict:
        return M.apply(self.o.read_state(), *self.o.read_log(), self.mach, self.R, self.cap, self.W, g0, n, replica)

    def restart(self, mask=None, *, ppm=None, g0=0, n=None, amnesia=False, replay=False, down_steps=0) -> dict:
        assert (mask is None) != (ppm is None)
        n = (self.G - g0 if mask is None else len(mask)) if n is None else n
        sel = select_mask(mask, self.R) if mask is not None else \
            select_random(int(self.p.seed), self.step_index, int(self.p.g0) + g0, n, self.R, ppm)
        before = self.o.read_state(g0, n)
        for j, r in np.argwhere(sel):
            self.hits["leader"] += int(fld(before, self.R, r, "role")[j] == abi.LEADER)
            self.hits["committed"] += int(fld(before, self.R, r, "commit")[j] > 0)
        per_group = sel.sum(axis=1)
        self.hits["two"] += int((per_group == 2).sum()) if self.R > 2 else 0
        self.hits["all"] += int((per_group == self.R).sum())
        self.hits["restarted"] += int(sel.sum())
        self.hits["spared"] += int((~sel).sum())
        heads = self.mach.heads() if self.mach else None
        info = restart_engine_like(self.o, sel, g0=g0, flags=(AMNESIA if amnesia else 0) | (REPLAY if replay else 0),
                                   down_steps=down_steps, applied=self.cursor, heads=heads,
                                   regs=self.mach.reg if self.mach else None)
        if self.mach:
            self.mach.applied[:], self.mach.lost[:], self.mach.hash[:] = heads["applied"], heads["lost"], heads["hash"]
        return info


# ---- the parity scenario shared by test_restart_cpu.py (non-vacuity, on the
# oracle alone) and test_gpu_restart.py (the engine against it)

PARITY_SLOTS = 4
# (R, G): 69 replicas at R = 3 make the second wave partial; the restarts cover groups [3, G - 2), unaligned at both
# ends (empty at R = 1, G = 5: the n == 0 call); (1, 70) puts R = 1 on two waves
PARITY_SHAPES = [(3, 23), (5, 203), (7, 10), (8, 9), (1, 5), (1, 70)]
PARITY_CASES = [(R, G, v) for R, G in PARITY_SHAPES for v in ("flat", "ring") + (("textbook",) if R == 5 else ())]
PARITY_FLAGS = [(0, 0), (0, 6), (REPLAY, 0), (REPLAY, 6), (AMNESIA, 0), (AMNESIA, 6)]     # (flags, down_steps)


# the random form: the engine's shard ends at global id 2^32 - 1, restarted at step 40 and again at step 80
RANDOM_KW = dict(R=5, G=203, g0=(1 << 32) - 203, seed=11, log_cap=300, **STRESS_MIX)
RANDOM_PPM = (0, 150_000, 1_000_000)
# the safety-observer run: textbook mode, flat log, drops, churn, partitions and commands, restarts every 20 steps
SAFETY_KW = dict(R=5, G=203, seed=11, log_cap=300, mode=abi.MODE_TEXTBOOK, ae_max_entries=4, **STRESS_MIX)
SAFETY_STEPS, SAFETY_PPM, SAFETY_SLOTS = 200, 100_000, 8


def parity_kw(R: int, G: int, variant: str) -> dict:
    extra = {"ring": dict(log_window=16), "textbook": dict(mode=abi.MODE_TEXTBOOK, ae_max_entries=4), "flat": {}}[variant]
    return dict(R=R, G=G, seed=11, log_cap=300, **extra, **STRESS_MIX)


def parity_mask(R: int, G: int, rnd: int) -> np.ndarray:
    """The mask bytes of restart number `rnd` over groups [3, G - 2): a third of
    the groups untouched, a third with random replicas (bits at or above R set
    too: ignored), every fifth group all of them."""
    n = max(G - 5, 0)
    rng = np.random.default_rng(1000 * R + 10 * G + rnd)
    m = rng.integers(0, 256, n, dtype=np.uint8)
    m[rng.random(n) < 1 / 3] = 0
    m[rnd::5] = 0xFF
    return m


def parity_run(x, flags: int, down_steps: int, label: str = "") -> list:
    """The scenario on `x` (a Host, or a RaftEngine with the machine
    configured): 40 steps, restart, 40 steps, restart, 40 steps, the consumers
    run after every leg.  Returns the checkpoints, each a dict of everything
    that must be equal between the engine and the oracle."""
    out = []

    def snap(what, **more):
        st = x.read_state()
        heads, regs = x.sm_read()
        out.append(dict(what=what, state=st, logs=x.read_log(), digest=x.digest(), applied=x.applied(), heads=heads,
                        regs=regs, **more))

    for leg in range(3):
        counters = x.step(40)
        rec, dinfo = x.drain_committed()
        snap(f"{label} leg {leg}", counters=counters, records=rec, drain=dinfo, apply=x.sm_apply())
        if leg < 2:
            info = x.restart(parity_mask(x.R, x.G, leg), g0=3,
                             amnesia=bool(flags & AMNESIA), replay=bool(flags & REPLAY), down_steps=down_steps)
            snap(f"{label} restart {leg}", info=info)
    return out


@functools.lru_cache(maxsize=None)
def host_parity_run(R: int, G: int, variant: str, flags: int, down_steps: int):
    """parity_run on the oracle, once per input and shared: (checkpoints, hits,
    every counter row).  Treat it as read-only."""
    h = Host(PARITY_SLOTS, **parity_kw(R, G, variant))
    points = parity_run(h, flags, down_steps, f"R{R} G{G} {variant}")
    h.close()
    return points, dict(h.hits), np.concatenate([p["counters"] for p in points if "counters" in p])


def valid_rows(counters: np.ndarray) -> int:
    """The leading counter rows of the oracle before its first
    RAFT_C_LOG_WINDOW_MISS.  From that step on a log_window run is invalid by
    the engine's contract (include/raft_engine.h raft_params.log_window): the
    oracle keeps every slot and reads what the ring no longer holds.  It
    happens here because a restarted replica has commitIndex 0, and the
    reference's new leader starts at nextIndex = commitIndex + 1 (quirk Q8):
    it replays from index 0, below every 16-slot window."""
    miss = np.flatnonzero(counters[:, abi.C_INDEX["log_window_miss"]])
    return int(miss[0]) if len(miss) else len(counters)


def assert_same_rows(got: np.ndarray, want: np.ndarray, label: str) -> bool:
    """The engine's counter rows equal the oracle's up to the oracle's first
    window miss, where the engine counts a miss too; True if there was none."""
    v = valid_rows(want)
    if not np.array_equal(got[:v], want[:v]):
        s, c = np.argwhere(got[:v] != want[:v])[0]
        raise AssertionError(f"{label}: counter {abi.COUNTER_NAMES[c]} differs at step {s} of the leg: "
                             f"{got[s, c]} vs {want[s, c]}")
    if v < len(want):
        assert got[v, abi.C_INDEX["log_window_miss"]] > 0, f"{label}: the engine counts no window miss at step {v}"
    return v == len(want)


def assert_same_points(got: list, want: list, R: int):
    """Every checkpoint of the engine's parity_run equals the oracle's, bit for
    bit, as long as the run is valid: on a ring, up to the first step in which
    the oracle counts a window miss (valid_rows); a flat log has none."""
    assert len(got) == len(want)
    for a, b in zip(got, want):
        label = b["what"]
        if "counters" in b and not assert_same_rows(a["counters"], b["counters"], label):
            return
        for k in ("info", "drain", "apply"):
            assert a.get(k) == b.get(k), f"{label}: {k} {a.get(k)} vs {b.get(k)}"
        if "counters" in b:
            assert np.array_equal(a["records"], b["records"]), f"{label}: drained records differ"
        assert_same_state(a["state"], b["state"], R, label)
        assert_same_logs(a["state"], a["logs"], b["logs"], R, label)
        assert a["digest"] == b["digest"], f"{label}: digest differs with equal state and logs"
        assert np.array_equal(a["applied"], b["applied"]), f"{label}: lastApplied differs"
        assert np.array_equal(a["heads"], b["heads"]), f"{label}: machine heads differ"
        assert np.array_equal(a["regs"], b["regs"]), f"{label}: machine registers differ"
