"""Snapshot install restated in numpy over the canonical words, logs, heads and
registers (include/raft_engine.h, raft_engine_install_snapshot*): the reference
of test_snapshot_cpu.py (over the oracle) and test_gpu_snapshot.py (against the
engine's kernel).  Nothing here touches a device."""
from __future__ import annotations

import functools

import numpy as np

import restart_model as RM
import sm_model as M
from helpers import F, abi, assert_same_logs, assert_same_state, fld

NF = abi.NUM_FIELDS
INFO_KEYS = ("installed", "slots_copied", "no_leader", "leader_gapped", "ahead")
HIT_KEYS = ("ex_leader", "shorter", "equal", "ahead", "lag_skipped", "no_leader", "one_leader", "two_leaders",
            "ring_short", "ring_full", "flat_over_64")


def newest_leader(w: np.ndarray, R: int):
    """(L, T) of one group's words: the replica with role LEADER and the highest
    currentTerm, the lowest index among equals; (-1, 0) without one."""
    L, T = -1, 0
    for r in range(R):
        if w[r * NF + F["role"]] == abi.LEADER and (L < 0 or w[r * NF + F["term"]] > T):
            L, T = r, int(w[r * NF + F["term"]])
    return L, T


def install(state, terms, cmds, heads, regs, sel, *, R: int, cap: int, W: int, seed: int, step: int, gid0: int,
            emin: int, emax: int, min_lag: int = 0, hits: dict | None = None, installed: list | None = None) -> dict:
    """Install the eligible replicas sel [n, R] of the n groups in `state`
    [n, words] (global ids gid0 ..), in place; terms / cmds [n, R, cap] are their
    logs as read_log gives them, heads [n, R] of abi.SM_HEAD_DTYPE and regs
    [n, R, S] their machines.  Returns the info; `hits` counts what it met and
    `installed` collects (j, L, f) of every install."""
    n = state.shape[0]
    assert sel.shape == (n, R) and min_lag >= 0
    info = dict.fromkeys(INFO_KEYS, 0)
    hit = dict.fromkeys(HIT_KEYS, 0) if hits is None else hits
    for j in range(n):
        w = state[j]
        L, T = newest_leader(w, R)
        if L < 0:
            info["no_leader"] += 1
            hit["no_leader"] += 1
            continue
        if heads[j, L]["lost"] != 0:
            info["leader_gapped"] += 1
            continue
        lastL, physL = int(w[L * NF + F["last"]]), int(w[L * NF + F["phys"]])
        hi = max(0, min(int(w[L * NF + F["commit"]]), lastL, cap))
        floor = max(0, physL - W) if W else 0
        nlead = sum(int(w[r * NF + F["role"]] == abi.LEADER) for r in range(R))
        done = 0
        for f in range(R):
            if not sel[j, f] or f == L:
                continue
            term_f, last_f = int(w[f * NF + F["term"]]), int(w[f * NF + F["last"]])
            if term_f > T:
                info["ahead"] += 1
                hit["ahead"] += 1
                continue
            if lastL - last_f < min_lag:
                hit["lag_skipped"] += 1
                continue
            hit["ex_leader"] += int(w[f * NF + F["role"]] == abi.LEADER and term_f < T)
            hit["shorter"] += int(last_f < lastL)
            hit["equal"] += int(last_f == lastL)
            hit["ring_short"] += int(bool(W) and physL < W)
            hit["ring_full"] += int(bool(W) and physL >= W)
            hit["flat_over_64"] += int(not W and physL > 64)
            done += 1
            if installed is not None:
                installed.append((j, L, f))
            info["installed"] += 1
            info["slots_copied"] += physL - floor
            # the log: the leader's retained slots (what read_log shows of its row)
            terms[j, f] = terms[j, L]
            cmds[j, f] = cmds[j, L]
            w[f * NF + F["last"]] = lastL
            w[f * NF + F["phys"]] = physL
            w[f * NF + F["commit"]] = hi
            if term_f != T:
                w[f * NF + F["voted"]] = -1
            w[f * NF + F["term"]] = T
            # the volatile state, as restart_model.restart
            w[f * NF + F["role"]] = abi.FOLLOWER
            w[f * NF + F["flags"]] = abi.FL_ARMED
            w[f * NF + F["phase_ms"]] = 0
            w[f * NF + F["retry_ms"]] = 0
            w[f * NF + F["election_ms"]] = RM.scale_range(RM.rng_word(seed, step, gid0 + j, abi.RNG_TIMER, f), emin, emax)
            w[R * NF + f * R:R * NF + (f + 1) * R] = 0                       # next[f][*]
            w[R * NF + R * R + f * R:R * NF + R * R + (f + 1) * R] = 0       # match[f][*]
            # the leader's session towards f
            w[R * NF + L * R + f] = lastL + 1
            w[R * NF + R * R + L * R + f] = lastL
            # the machine
            heads[j, f] = heads[j, L]
            regs[j, f] = regs[j, L]
        if done:
            hit["one_leader" if nlead == 1 else "two_leaders"] += 1
    return info


def install_engine_like(x, sel, *, g0: int, min_lag: int = 0, hits: dict | None = None) -> dict:
    """The host route on anything with read_state / read_log / sm_read and their
    writes, step_index and raft_params `p` (the Host below, or a RaftEngine):
    read -> model -> write_state, write_log, sm_write of groups [g0, g0 + len(sel))."""
    n = sel.shape[0]
    st = x.read_state(g0, n)
    t, c = x.read_log(g0, n)
    heads, regs = x.sm_read(g0, n)
    info = install(st, t, c, heads, regs, sel, R=x.R, cap=int(x.p.log_cap), W=int(x.p.log_window), seed=int(x.p.seed),
                   step=int(x.step_index), gid0=int(x.p.g0) + g0, emin=int(x.p.election_min_ms),
                   emax=int(x.p.election_max_ms), min_lag=min_lag, hits=hits)
    x.write_state(st, g0)
    x.write_log(t, c, g0)
    x.sm_write(heads, regs, g0)
    return info


class Host(RM.Host):
    """restart_model.Host (the oracle with apply_model's cursor and sm_model's
    machine beside it) with the install under RaftEngine's method names:
    install_snapshot is read -> install() above -> write_state / write_log, the
    machine's words stored in the model.  `ihits` counts what the installs met
    (the non-vacuity conditions of test_snapshot_cpu.py)."""

    def __init__(self, slots: int, **kw):
        super().__init__(slots, **kw)
        self.ihits = dict.fromkeys(HIT_KEYS, 0)

    def write_state(self, st, g0=0):
        self.o.write_state(st, g0)

    def write_log(self, t, c, g0=0):
        self.o.write_log(t, c, g0)

    def sm_read(self, g0=0, n=None):
        n = self.G - g0 if n is None else n
        return self.mach.heads(g0, n), self.mach.reg[g0:g0 + n].copy()

    def sm_write(self, heads, regs, g0=0):
        n = heads.shape[0]
        self.mach.applied[g0:g0 + n], self.mach.lost[g0:g0 + n] = heads["applied"], heads["lost"]
        self.mach.hash[g0:g0 + n], self.mach.reg[g0:g0 + n] = heads["hash"], regs

    def install_snapshot(self, mask=None, *, g0=0, n=None, min_lag=0, device_mask=None) -> dict:
        assert device_mask is None
        n = (self.G - g0 if mask is None else len(mask)) if n is None else n
        sel = RM.select_mask(mask, self.R) if mask is not None else np.ones((n, self.R), bool)
        if n == 0:
            return dict.fromkeys(INFO_KEYS, 0)
        return install_engine_like(self, sel, g0=g0, min_lag=min_lag, hits=self.ihits)

    def heal(self, min_lag=None) -> dict:
        """RaftService.heal: an sm_apply of everything, then an install of every group."""
        if min_lag is None:
            min_lag = self.W // 2 if self.W else self.cap // 4
        self.sm_apply()
        return self.install_snapshot(min_lag=min_lag)


# ---- the parity scenario shared by test_snapshot_cpu.py (non-vacuity, on the
# oracle alone) and test_gpu_snapshot.py (the engine against it)

def install_mask(R: int, G: int, rnd: int) -> np.ndarray:
    """The mask bytes of the first install over groups [3, G - 2): random
    replicas (bits at or above R set too: ignored), a quarter of the groups
    untouched, every fifth group all of them."""
    n = max(G - 5, 0)
    rng = np.random.default_rng(7000 * R + 13 * G + rnd)
    m = rng.integers(0, 256, n, dtype=np.uint8)
    m[rng.random(n) < 1 / 4] = 0
    m[rnd::5] = 0xFF
    return m


# the legs' lengths: both installs fall into the last steps of a partition of STRESS_MIX (steps 80-89 and 160-169),
# when deposed leaders still hold the role LEADER, and the second late enough for flat logs of more than 64 slots
PARITY_LEGS = (40, 48, 80, 40)


def parity_run(x, label: str = "") -> list:
    """The scenario on `x` (a Host, or a RaftEngine with the machine
    configured): 40 steps, a REPLAY restart by restart_model.parity_mask with
    down_steps 6, 48 steps, sm_apply, an install over [3, G - 2) by
    install_mask, 80 steps, an install of everything with min_lag 4, 40 steps;
    the consumers run after every leg.  Returns the checkpoints, each a dict of
    everything that must be equal between the engine and the oracle."""
    out = []

    def snap(what, **more):
        heads, regs = x.sm_read()
        out.append(dict(what=what, state=x.read_state(), logs=x.read_log(), digest=x.digest(), applied=x.applied(),
                        heads=heads, regs=regs, **more))

    def leg(k):
        counters = x.step(PARITY_LEGS[k])
        rec, dinfo = x.drain_committed()
        snap(f"{label} leg {k}", counters=counters, records=rec, drain=dinfo, apply=x.sm_apply())

    leg(0)
    snap(f"{label} restart", info=x.restart(RM.parity_mask(x.R, x.G, 0), g0=3, replay=True, down_steps=6))
    leg(1)
    snap(f"{label} masked install", info=x.install_snapshot(install_mask(x.R, x.G, 1), g0=3))
    leg(2)
    snap(f"{label} install of all", info=x.install_snapshot(min_lag=4))
    leg(3)
    return out


@functools.lru_cache(maxsize=None)
def host_parity_run(R: int, G: int, variant: str):
    """parity_run on the oracle, once per input and shared: (checkpoints, hits,
    every counter row).  Treat it as read-only."""
    h = Host(RM.PARITY_SLOTS, **RM.parity_kw(R, G, variant))
    points = parity_run(h, f"R{R} G{G} {variant}")
    h.close()
    return points, dict(h.ihits), np.concatenate([p["counters"] for p in points if "counters" in p])


# ---- an installed ex-leader, built by hand: the stress mix never leaves a deposed leader with a shorter log
EX_LEADER_KW = dict(R=5, G=9, seed=4, log_cap=64, cmd_ppm=1_000_000)


def craft_ex_leader(x, steps: int = 60):
    """Step `x` (a Host or a RaftEngine with the machine configured), apply, and
    rewrite one follower of the first group whose leader has three
    entries into a deposed leader: role LEADER, the term before the leader's, its
    own vote, a log two entries shorter.  Returns (group, leader, that replica)."""
    x.step(steps)
    x.sm_apply()
    st = x.read_state()
    R = x.R
    for g in range(st.shape[0]):
        L, T = newest_leader(st[g], R)
        if L >= 0 and T >= 1 and st[g, L * NF + F["last"]] >= 3:
            break
    else:
        raise AssertionError("no group with a leader and three entries")
    f = (L + 1) % R
    w = st[g]
    short = min(int(w[f * NF + F["last"]]), int(w[L * NF + F["last"]]) - 2)
    w[f * NF + F["term"]], w[f * NF + F["voted"]], w[f * NF + F["role"]] = T - 1, f, abi.LEADER
    w[f * NF + F["last"]] = w[f * NF + F["phys"]] = short
    x.write_state(st)
    return g, L, f


# ---- the validity scenario: a ring that stays valid because lagging replicas are healed
#
# Textbook mode, R = 5, G = 203, W = 16, S = 8, no drops, churn or partitions, a
# command every step (40 entries in 40 steps, far more than W).  Persistent
# restarts at 10^5 ppm with down_steps 40 every 60 steps for 240 steps, after a
# warm-up that elects the first leaders.  What the oracle showed while this was
# set up, and why the schedule is what it is:
# - The textbook leader builds every request from its own log[nextIndex - 2],
#   also towards a replica that is cut off.  nextIndex towards an isolated
#   replica stands still, so the leader reads below its window W appended entries
#   into the isolation, long before it ends.  A heal at the isolation's end alone
#   cannot keep the run valid; the healed run heals every VALID_HEAL steps, the
#   isolations' ends among them (the install ignores the isolation word: a
#   teleport).  With min_lag = W / 2 = 8 and a command a step no replica is ever
#   more than 8 + VALID_HEAL - 1 = 12 entries behind, inside the window.
# - An isolated replica whose election timer fires climbs to terms above the
#   leader's and is skipped as `ahead`; nothing can heal it until the group has
#   caught up with its term.  The election timeouts are therefore longer (50 to
#   57.5 steps) than the isolation (40 steps).
# - A machine that applies nothing for more than W entries is GAPPED, and a
#   gapped leader installs nothing: heal's sm_apply runs from the first step on.
VALID_KW = dict(R=5, G=203, seed=11, log_cap=512, log_window=16, mode=abi.MODE_TEXTBOOK, ae_max_entries=4,
                cmd_ppm=1_000_000, election_min_ms=100_000, election_max_ms=115_000)
VALID_SLOTS, VALID_PPM, VALID_DOWN, VALID_EVERY, VALID_STEPS = 8, 100_000, 40, 60, 240
VALID_WARM, VALID_HEAL = 80, 5


def validity_run(x, heal, label: str = "") -> dict:
    """VALID_WARM steps, then persistent restarts at VALID_PPM with down_steps
    VALID_DOWN every VALID_EVERY steps for VALID_STEPS steps on `x` (a Host, or
    a RaftEngine with the machine configured); heal(x), if given, is called
    every VALID_HEAL steps.  Returns the counter rows, the infos and the final
    words."""
    rows, infos = [], []

    def steps(k):
        for _ in range(k // VALID_HEAL if heal is not None else 1):
            rows.append(x.step(VALID_HEAL if heal is not None else k))
            if heal is not None:
                infos.append(heal(x))

    steps(VALID_WARM)
    for _ in range(VALID_STEPS // VALID_EVERY):
        infos.append(x.restart(ppm=VALID_PPM, down_steps=VALID_DOWN))
        steps(VALID_EVERY)
    infos.append(x.sm_apply())
    heads, regs = x.sm_read()
    return dict(counters=np.concatenate(rows), infos=infos, state=x.read_state(), logs=x.read_log(), digest=x.digest(),
                heads=heads, regs=regs)


@functools.lru_cache(maxsize=None)
def host_validity_run(healed: bool):
    """validity_run on the oracle, with or without the heal, once and shared:
    (the run, the installs' hits, the final Machine).  Treat it as read-only."""
    h = Host(VALID_SLOTS, **VALID_KW)
    run = validity_run(h, (lambda x: x.heal()) if healed else None)
    h.close()
    return run, dict(h.ihits), h.mach


def assert_same_run(got: dict, want: dict, R: int, label: str):
    """Two validity_runs are equal bit for bit (a run without a window miss)."""
    assert np.array_equal(got["counters"], want["counters"]), f"{label}: counter rows differ"
    assert got["infos"] == want["infos"], f"{label}: infos {got['infos']} vs {want['infos']}"
    assert_same_state(got["state"], want["state"], R, label)
    assert_same_logs(got["state"], got["logs"], want["logs"], R, label)
    assert got["digest"] == want["digest"], f"{label}: digest differs with equal state and logs"
    assert np.array_equal(got["heads"], want["heads"]) and np.array_equal(got["regs"], want["regs"]), f"{label}: machine"
