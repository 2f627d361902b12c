"""The log-tail cache as the log defines it: the reference of
tests/test_gpu_tail_cache.py, checked by tests/test_tail_cache_cpu.py.

Every replica carries three words beside its canonical fields (FIELD_SLOT 6, 9
and 10 of csrc/raft_step.h): t1 and t2, the terms of log[last - 1] and
log[last - 2], and c1, the command of log[last - 1].  Eight kinds of device
code write them, each with an update of its own; `derive` restates the one rule
they all have to agree with, rebuild_cache_kernel's (csrc/raft_engine.hip):

    t1, c1 = term, cmd of slot last - 1   if last >= 1, else 0
    t2     = term of slot last - 2        if last >= 2, else 0

`defined` marks the words whose slot the replica still retains: index >=
max(0, physLen - W).  On a flat log (W = 0) that is every word.  On a
log_window ring a slot below the window has been overwritten by a newer index
(the ring aliases), so no rule says what the word holds and the comparison
leaves it out.  How many words that excludes is a condition on a test's inputs,
computed on the oracle's or the model's state, never on the engine under test:
0 on a flat log, at most EXCLUDED_MAX of the words on a ring.

Nothing here is narrowed for a particular writer: a word whose index is
negative (t2 at last <= 1, all three at last == 0) is defined, and is 0.
"""
from __future__ import annotations

import numpy as np

from helpers import abi, fld

WORDS = ("t1", "t2", "c1")
EXCLUDED_MAX = 0.01          # the share of undefined words a ring case may have


def _cols(state: np.ndarray, R: int, name: str) -> np.ndarray:
    """Field `name` of every replica: [n, R]."""
    return np.stack([fld(state, R, r, name) for r in range(R)], axis=1).astype(np.int64)


def derive(state: np.ndarray, terms: np.ndarray, cmds: np.ndarray, R: int, W: int = 0) -> np.ndarray:
    """The cache the logs define: [n, R, 3] int32 (t1, t2, c1; c1's bits as
    int32, as the engine stores them).  terms / cmds are read_log's image
    [n, R, log_cap], indexed by log index (W does not change where an index
    lies in the image; `defined` says which of the words mean something)."""
    last = _cols(state, R, "last")
    cap = terms.shape[2]
    out = np.zeros(last.shape + (3,), dtype=np.int32)
    for k, (back, src) in enumerate(((1, terms), (2, terms), (1, cmds))):
        i = last - back
        v = np.take_along_axis(np.asarray(src), np.clip(i, 0, cap - 1)[:, :, None], axis=2)[:, :, 0]
        out[:, :, k] = np.where(i >= 0, v.astype(np.int64) & 0xFFFFFFFF, 0).astype(np.uint32).view(np.int32)
    return out


def defined(state: np.ndarray, R: int, W: int = 0) -> np.ndarray:
    """[n, R, 3] bool: the word's slot is retained (or the word is the 0 of a
    negative index).  W = 0: a flat log, everything."""
    last, phys = _cols(state, R, "last"), _cols(state, R, "phys")
    lo = np.maximum(0, phys - W) if W else np.zeros_like(phys)
    out = np.ones(last.shape + (3,), dtype=bool)
    for k, back in enumerate((1, 2, 1)):
        i = last - back
        out[:, :, k] = (i < 0) | (i >= lo)
    return out


def excluded_share(state: np.ndarray, R: int, W: int = 0) -> float:
    """The share of the words `defined` leaves out (of an oracle's or a model's state)."""
    d = defined(state, R, W)
    return float(np.count_nonzero(~d)) / max(1, d.size)


def assert_condition(state: np.ndarray, R: int, W: int, label: str = "") -> float:
    """The exclusion condition of a case, on the reference's state: 0 on a
    flat log, at most EXCLUDED_MAX on a ring.  Returns the share."""
    share = excluded_share(state, R, W)
    assert share == 0.0 if not W else share <= EXCLUDED_MAX, f"{label}: {share:.4%} of the cache words are below the window"
    return share


def first_mismatch(cache: np.ndarray, state: np.ndarray, terms: np.ndarray, cmds: np.ndarray, R: int, W: int = 0):
    """None when cache equals derive(...) on every defined word; else a
    description of the first word that does not: group, replica, word, last, phys."""
    want, ok = derive(state, terms, cmds, R, W), defined(state, R, W)
    bad = np.argwhere((np.asarray(cache) != want) & ok)
    if not len(bad):
        return None
    g, r, k = (int(x) for x in bad[0])
    return (f"{len(bad)} cache words differ from the log; first group {g} replica {r} word {WORDS[k]}: "
            f"{int(cache[g, r, k])} in HBM, {int(want[g, r, k])} in the log "
            f"(last {int(fld(state[g], R, r, 'last'))}, phys {int(fld(state[g], R, r, 'phys'))})")


def assert_cache(e, label: str, W: int | None = None):
    """The engine's cache is marked current and equals what its own state and
    logs define, word for word on the defined words.  Reads only; returns
    (state, cache)."""
    import importlib
    dbg = importlib.import_module("raft-kotlin_amd.debug")
    W = int(e.p.log_window) if W is None else W
    state = e.read_state()
    terms, cmds = e.read_log()
    cache, valid = dbg.read_tail_cache(e)
    assert valid == 1, f"{label}: the cache is marked stale"
    bad = first_mismatch(cache, state, terms, cmds, e.R, W)
    assert bad is None, f"{label}: {bad}"
    return state, cache


# ---- the call sequences ---------------------------------------------------------
# A scenario is a function of `x`, anything under RaftEngine's method names.  On
# the CPU it runs on a Recorder around a Host (the oracle with the side paths'
# models beside it): the Recorder writes down every call that is no plain read,
# with its result and with the excluded share of the state the call left.
# tests/test_tail_cache_cpu.py asserts the conditions on that; on the GPU
# tests/test_gpu_tail_cache.py makes the same calls, in the same order and with
# the same arguments, on an engine (play), compares the results and runs
# assert_cache after every device-side writer.

# calls that change nothing (never recorded)
READS = {"read_state", "read_log", "digest", "digest_range", "applied", "sm_read", "outbox_read", "outbox_len",
         "check_log_matching", "close"}
# calls after which the cache must be current and equal to the log: every device-side writer and consumer
WRITERS = {"step", "vote_batch", "append_batch", "append_command_batch", "propose", "append_noops", "outbox_pump",
           "restart", "install_snapshot", "replay", "transfer"}
# results that must be equal between the host and the engine, call by call
COMPARED = {"step", "vote_batch", "append_batch", "propose", "restart", "install_snapshot", "replay"}


def _host_vote_batch(h, grp, dst, vq):
    return np.array([h.o.vote(int(g), int(d), *map(int, q)) for g, d, q in zip(grp, dst, vq)], dtype=np.int32).reshape(-1, 2)


def _host_append_batch(h, grp, dst, aq):
    out = []
    for g, d, q in zip(grp, dst, aq):
        t, s, st = h.o.append(int(g), int(d), int(q[0]), int(q[1]), int(q[2]), int(q[3]),
                              (int(q[5]), int(q[6])) if q[4] else None, int(q[7]))
        out.append((t, int(s), st))
    return np.array(out, dtype=np.int32).reshape(-1, 3)


def _host_command_batch(h, grp, dst, cmd):
    for g, d, c in zip(grp, dst, cmd):
        h.o.append_command(int(g), int(d), int(c))


def _host_replay(h, rec, keep_volatile=False):
    import replay_model as RP
    st, (t, c) = h.read_state(), h.read_log()
    info = RP.replay_into(h, rec, st, t, c, keep_volatile)
    h.write_state(st)
    h.write_log(t, c)
    return info


def _engine_replay(e, rec, keep_volatile=False):
    import importlib
    return importlib.import_module("raft-kotlin_amd.replay").replay(e, rec, keep_volatile=keep_volatile)


HOST_CALLS = {"vote_batch": _host_vote_batch, "append_batch": _host_append_batch,
              "append_command_batch": _host_command_batch, "replay": _host_replay,
              "set_kernel": lambda h, k: None, "set_batch_path": lambda h, p: None}
ENGINE_CALLS = {"replay": _engine_replay}


class Recorder:
    """A Host under its own method names, every call that is no read written
    into `trace`: dict(name, args, kw, res, share, miss)."""

    def __init__(self, host):
        self.h, self.trace = host, []

    def __getattr__(self, name):
        h = self.__dict__["h"]
        if name in READS or (name not in HOST_CALLS and not callable(getattr(h, name))):
            return getattr(h, name)

        def call(*args, **kw):
            res = HOST_CALLS[name](h, *args, **kw) if name in HOST_CALLS else getattr(h, name)(*args, **kw)
            self.trace.append(dict(name=name, args=args, kw=kw, res=res, share=excluded_share(h.read_state(), h.R, h.W)))
            return res
        return call


def same(a, b) -> bool:
    if isinstance(a, dict) and isinstance(b, dict):
        return set(a) == set(b) and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)) and isinstance(b, (tuple, list)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return np.array_equal(np.asarray(a), np.asarray(b))
    return a == b


def play(e, trace, check, label: str = ""):
    """The recorded calls on the engine `e`; check(e, label) after every WRITER."""
    valid = True                                                  # no access below a window so far (the host's count):
    for k, c in enumerate(trace):                                 # from the first one on parity is not promised
        name = c["name"]
        fn = ENGINE_CALLS[name] if name in ENGINE_CALLS else None
        res = fn(e, *c["args"], **c["kw"]) if fn else getattr(e, name)(*c["args"], **c["kw"])
        what = f"{label} call {k} {name}"
        if name == "step" and _sum(c["res"], "log_window_miss"):
            valid = False
        if name in COMPARED and valid:
            assert same(res, c["res"]), f"{what}: the engine's result differs from the host's"
        if name in WRITERS:
            check(e, what)
    return valid


def make_host(sc):
    """The oracle under every method name the scenarios call: outbox_model's
    Host (steps, restarts, transfers, proposals, no-ops, the outbox) with
    snapshot_model's (write_state / write_log, install_snapshot) beside it."""
    import outbox_model as OM
    import snapshot_model as SM

    class Host(OM.Host, SM.Host):
        pass
    return Host(sc.get("slots", 0), **sc["kw"])


def ring16_kw(mode) -> dict:
    """RING16's faults in either mode.  Reference mode appends at the physical
    end, so ghost tails push lastIndex below a 16-slot window: its ring is 64."""
    kw = {k: v for k, v in RING16.items() if k not in ("mode", "ae_max_entries")}
    return dict(kw, mode=abi.MODE_TEXTBOOK, ae_max_entries=4) if mode else dict(kw, log_window=64)


_RUNS = {}


def host_run(name: str) -> dict:
    """Scenario `name` on the oracle, once and shared (read-only): the trace,
    the facts the scenario returned, the final state, logs and digest."""
    if name not in _RUNS:
        sc = SCENARIOS[name]
        h = make_host(sc)
        rec = Recorder(h)
        facts = sc["run"](rec) or {}
        _RUNS[name] = dict(trace=rec.trace, facts=facts, state=h.read_state(), logs=h.read_log(), digest=h.digest(),
                           W=h.W, R=h.R)
        h.close()
    return _RUNS[name]


def _cols_of(st, R, name):
    return _cols(st, R, name)


def _sum(rows, name):
    return int(np.asarray(rows)[:, abi.C_INDEX[name]].sum())


# ---- handler batches
def _handler_inputs(R, ring, n, seed, G=None, skew=False):
    from helpers import handler_messages, random_ring_states, random_states
    rng = np.random.default_rng(seed)
    W, cap = (64, 160) if ring else (0, 8)
    G = G or (2000 if ring else 64)
    w, lt, lc = random_ring_states(rng, G, R, cap, W) if ring else random_states(rng, G, R, cap)
    grp, dst, vq, aq, cmd = handler_messages(rng, n, G, R, cap, w, W)
    if skew:                                                      # test_handler_batches_skewed_vs_oracle's batch
        hot = rng.random(n) < 0.5
        grp, dst = np.where(hot, 7, grp), np.where(hot, 2, dst).astype(np.int32)
    return dict(R=R, G=G, log_cap=cap, log_window=W, seed=3), (w, lt, lc), (grp, dst, vq, aq, cmd)


def handlers(R, mode, ring, n, seed, G=None, skew=False):
    kw, (w, lt, lc), (grp, dst, vq, aq, cmd) = _handler_inputs(R, ring, n, seed, G, skew)

    def run(x):
        x.write_state(w)
        x.write_log(lt, lc)
        x.append_batch(grp, dst, aq)
        x.append_command_batch(grp, dst, cmd)
        st = x.read_state()
        return dict(wrapped=int(_cols_of(st, R, "phys").max()) > kw["log_window"] > 0,
                    ghost=int(np.count_nonzero(_cols_of(st, R, "phys") != _cols_of(st, R, "last"))))
    return dict(kw=dict(kw, mode=mode), run=run, paths=True)


# ---- the consumer sequence: what the batches stored back is read by a vote batch, by an append batch whose prev
# sits on the cached entries, and by the step kernel
CONSUMER_MIX = dict(cmd_ppm=500_000, drop_ppm=50_000)


def tail_appends(rng, st, terms, n, R):
    """n AppendEntries whose prevLogIndex is lastIndex - 1 or lastIndex - 2 of its
    target in `st` (the handler answers from t1 / t2), three in four with the
    term the log holds there, in the target's current term, half with an entry."""
    G = st.shape[0]
    grp, dst = rng.integers(0, G, n), rng.integers(0, R, n).astype(np.int32)
    last = st[grp, dst * abi.NUM_FIELDS + abi.F_INDEX["last"]].astype(np.int64)
    term = st[grp, dst * abi.NUM_FIELDS + abi.F_INDEX["term"]].astype(np.int64)
    prev = np.maximum(last - rng.integers(1, 3, n), -1)
    pt = np.where(prev >= 0, terms[grp, dst, np.maximum(prev, 0)], 0) + (rng.random(n) < 0.25)
    aq = np.stack([term, rng.integers(1, R + 1, n), prev, pt, rng.integers(0, 2, n), term,
                   rng.integers(0, 1 << 32, n, dtype=np.uint64), rng.integers(0, 8, n)], axis=1).astype(np.int64)
    return grp, dst, aq


def consumer(mode, ring):
    from helpers import handler_messages
    R, G, cap, W = 5, 64, 300, (16 if ring else 0)
    kw = dict(R=R, G=G, seed=11, log_cap=cap, log_window=W, mode=mode, **CONSUMER_MIX)

    def run(x):
        rows = [x.step(60)]
        w, (lt, lc) = x.read_state(), x.read_log()
        x.write_state(w)                                          # a host write: the first batch rebuilds the cache
        x.write_log(lt, lc)
        rng = np.random.default_rng(5 + W)
        grp, dst, vq, aq, cmd = handler_messages(rng, 600, G, R, cap, w, W)
        x.append_batch(grp, dst, aq)
        x.append_command_batch(grp, dst, cmd)
        x.vote_batch(grp, dst, vq)
        st, (t, _) = x.read_state(), x.read_log()
        g2, d2, aq2 = tail_appends(rng, st, t, 600, R)
        resp = x.append_batch(g2, d2, aq2)
        rows.append(x.step(20))
        return dict(rows=np.concatenate(rows), accepted=int(np.count_nonzero(resp[:, 1])),
                    refused=int(np.count_nonzero(resp[:, 1] == 0)),
                    wrapped=int(_cols_of(st, R, "phys").max()) > W > 0)
    return dict(kw=kw, run=run, paths=True)


# ---- the step kernel: a 1-step launch, a K-step launch, a second launch
def stepper(kw, k1, k2, setup=()):
    def run(x):
        for name, arg in setup:
            getattr(x, name)(arg)
        R = kw["R"]
        rows, ghost, shrunk = [], 0, 0
        for k in (1, k1, k2):
            before = _cols_of(x.read_state(), R, "last")
            rows.append(x.step(k))
            st = x.read_state()
            ghost += int(np.count_nonzero(_cols_of(st, R, "phys") != _cols_of(st, R, "last")))
            shrunk += int(np.count_nonzero(_cols_of(st, R, "last") < before))
        last = _cols_of(st, R, "last")
        return dict(rows=np.concatenate(rows), ghost=ghost, shrunk=shrunk, lag=int((last.max(1) - last.min(1)).max()),
                    wrapped=int(_cols_of(st, R, "phys").max()) > kw.get("log_window", 0) > 0)
    return dict(kw=kw, run=run)


def _net_kw(R, faults):
    """test_network_fault_kernels' parameters (tests/test_gpu_parity.py NET_CASES) at 203 groups."""
    kw = dict(R=R, G=203, seed=200 + R, log_cap=300, cmd_ppm=500_000)
    if "churn" in faults:
        kw.update(churn_ppm=20_000, churn_steps=15)
    if "drops" in faults:
        kw.update(drop_ppm=100_000)
    if "partitions" in faults:
        kw.update(partition_period=40, partition_len=10)
    if "all-leaders" in faults:
        kw.update(cmd_mode=abi.CMD_ALL_LEADERS)
    if "limit" in faults:
        kw.update(cmd_limit=30)
    return kw


NET_CASES = [(3, "drops+churn"), (5, "drops+churn"), (7, "drops+churn"), (5, "drops"), (3, "partitions"),
             (5, "partitions"), (7, "partitions"), (7, "partitions+churn"), (5, "none"), (5, "churn"),
             (5, "drops+all-leaders"), (5, "drops+limit")]
# a ring of 16 under faults mild enough that no access falls below the window (tests/test_gpu_replay.py's ring)
RING16 = dict(R=5, G=203, seed=11, log_cap=512, mode=abi.MODE_TEXTBOOK, ae_max_entries=4, cmd_ppm=250_000,
              drop_ppm=50_000, partition_period=150, partition_len=10, log_window=16)


def _step_scenarios():
    import restart_model as RM
    import tick_paths_model as TP
    from helpers import STRESS_MIX
    out = {}
    for R in range(1, 9):
        out[f"step-ref-R{R}"] = stepper(RM.parity_kw(R, 203, "flat"), 60, 60)
    for E in (1, 3, 8):
        out[f"step-tb-E{E}"] = stepper(dict(R=5, G=203, seed=11, log_cap=300, mode=abi.MODE_TEXTBOOK, ae_max_entries=E,
                                            **STRESS_MIX), 60, 60)
    out["step-ring16"] = stepper(RING16, 150, 60)
    out["step-ring64"] = stepper(dict(R=5, G=203, seed=105, log_cap=300, log_window=64, **STRESS_MIX), 100, 60)
    for R, f in NET_CASES:
        out[f"step-net-{R}-{f}"] = stepper(_net_kw(R, f), 60, 60)
    out["step-general"] = stepper(RM.parity_kw(5, 203, "flat"), 60, 60, setup=(("set_kernel", abi.KERNEL_GENERAL),))
    c3 = dict(abi.CONFIGS[3], churn_ppm=10_000)
    out["step-balanced"] = stepper(dict(c3, G=4000, log_cap=200, steps_per_launch=37, schedule=abi.SCHED_BALANCED,
                                        schedule_workgroups=7), 37, 37)
    out["step-epochs"] = stepper(dict(c3, G=1000, log_cap=900, log_window=64, steps_per_launch=1000,
                                      schedule=abi.SCHED_BALANCED), 700, 60)
    for mode in (abi.MODE_REFERENCE, abi.MODE_TEXTBOOK):
        out[f"step-overflow-{'tb' if mode else 'ref'}"] = stepper(
            dict(abi.CONFIGS[3], G=500, churn_ppm=20_000, cmd_ppm=1_000_000, log_cap=40, mode=mode), 150, 150)
    for R, W in TP.CATCH_UP:                                      # the states whose ticks read past the tail cache
        sc = TP.catch_up(R, W)
        out[f"step-catchup-R{R}-{'ring' if W else 'flat'}"] = stepper(sc["kw"], sc["steps"] - 21, 20)
    return out


# ---- the client writers: the image loaded, one step (the cache is current), the call
def client(kind, mode, ring):
    import outbox_model as OM
    kw = ring16_kw(mode) if ring else OM.parity_kw(5, "textbook" if mode else "reference", "flat")

    def run(x):
        x.step(40)
        w, (lt, lc) = x.read_state(), x.read_log()
        x.write_state(w)
        x.write_log(lt, lc)
        x.step(1)
        G = x.G
        facts = {}
        if kind == "propose":
            groups = np.concatenate([np.arange(G), np.arange(0, G, 3)]).astype(np.int64)
            tk = x.propose(groups, (5000 + np.arange(len(groups))).astype(np.uint32))
            facts = {n: int(np.count_nonzero(tk["status"] == i)) for i, n in enumerate(abi.PROPOSE_STATUS_NAMES)}
        elif kind == "noops":
            facts = dict(x.append_noops(cmd=0xFFFF0001))
        x.step(5)
        return facts
    return dict(kw=kw, run=run)


def crafted_client(kind, mode):
    """The crafted images of client_model / noop_model: a leader with a ghost tail, a leader whose log is full."""
    import client_model as CM
    import noop_model as NM
    w, t, c = CM.crafted() if kind == "propose" else NM.crafted()
    G, R, cap = t.shape
    kw = dict(R=R, G=G, log_cap=cap, mode=mode)

    def run(x):
        x.write_state(w)
        x.write_log(t, c)
        x.step(1)
        if kind == "propose":
            before = x.read_state()
            tk = x.propose(CM.CRAFTED_GROUPS, CM.CRAFTED_CMDS)
            facts = {n: int(np.count_nonzero(tk["status"] == i)) for i, n in enumerate(abi.PROPOSE_STATUS_NAMES)}
            facts["ghost_before"] = int(np.count_nonzero(_cols_of(before, R, "phys") != _cols_of(before, R, "last")))
            return facts
        return dict(x.append_noops(cmd=NM.NOOP))
    return dict(kw=kw, run=run)


def outbox(mode, ring):
    import outbox_model as OM
    kw = ring16_kw(mode == "textbook") if ring == "ring" else OM.parity_kw(5, mode, "flat")

    def run(x):
        points = OM.parity_run(x, "outbox")
        return dict(OM.totals(points))
    return dict(kw=kw, run=run)


# ---- restart, install, replay
def restarts(variant, flags):
    import restart_model as RM
    kw = RING16 if variant == "ring" else RM.parity_kw(5, 203, variant)

    def run(x):
        amnesia, rp = bool(flags & RM.AMNESIA), bool(flags & RM.REPLAY)
        x.step(40)
        mask = RM.parity_mask(x.R, x.G, 0)
        before = x.read_state()
        info = x.restart(mask, g0=3, amnesia=amnesia, replay=rp)
        after = x.read_state()
        x.step(20)
        info2 = x.restart(ppm=150_000, amnesia=amnesia, replay=rp)          # the random form
        x.step(20)
        sel = np.zeros((x.G, x.R), bool)
        sel[3:3 + len(mask)] = RM.select_mask(mask, x.R)
        last0, last1 = _cols_of(before, x.R, "last"), _cols_of(after, x.R, "last")
        return dict(restarted=info["restarted"], random=info2["restarted"], spared=int((~sel).sum()),
                    kept=bool(np.array_equal(last0[~sel], last1[~sel])),
                    emptied=int(np.count_nonzero((last0 > 0) & (last1 == 0))))
    return dict(kw=kw, run=run, slots=RM.PARITY_SLOTS)


def installs(ring):
    import restart_model as RM
    import snapshot_model as SM
    kw = dict(RING16, cmd_ppm=1_000_000) if ring else RM.parity_kw(5, 203, "flat")

    def run(x):
        for _ in range(15):                                                 # the machine keeps up: no gapped leader
            x.step(10)
            x.sm_apply()
        x.restart(RM.parity_mask(x.R, x.G, 0), g0=3, amnesia=True)          # replicas that lag by their whole log
        if ring:                                                            # every emptied replica is healed at once:
            i1 = x.install_snapshot(min_lag=4)                              # a leader never reads below its window
        else:
            x.step(3)
            x.sm_apply()
            i1 = x.install_snapshot(SM.install_mask(x.R, x.G, 1), g0=3)
        x.step(5 if ring else 30)
        x.sm_apply()
        i2 = x.install_snapshot(SM.install_mask(x.R, x.G, 1), g0=3) if ring else x.install_snapshot(min_lag=4)
        x.step(5 if ring else 20)
        return dict(installed=i1["installed"] + i2["installed"], **dict(x.ihits))
    return dict(kw=kw, run=run, slots=RM.PARITY_SLOTS)


def _run_records(g, r, term, vote, keep, entries):
    import wal_model as WM
    rows = [(g, r, WM.HS, -1, term, 0, vote)] if term is not None else []
    if keep is not None:
        rows.append((g, r, WM.TR, keep, 0, 0, 0))
    rows += [(g, r, WM.EN, i, t, c, 0) for i, t, c in entries]
    return rows


def replays(ring):
    """raft_wal_replay on an engine's own replicas, the batches built from the
    state the oracle holds: groups [0, 50) and [70, 100) whole (HARDSTATE, TRUNCATE, ENTRYs),
    [50, 70) the same cut into pieces of 7 records (inside the runs), [100, 130)
    runs that end in a TRUNCATE with keep 0, 1 and 2, [130, 160) lone
    HARDSTATEs, [160, 200) whole with KEEP_VOLATILE, and on a flat log one
    replica of group 200 with a run of 580 ENTRYs (more than one workgroup)."""
    import wal_model as WM
    W = 16 if ring else 0
    kw = dict(RING16, log_cap=600) if ring else dict(R=5, G=203, seed=11, log_cap=600, mode=abi.MODE_TEXTBOOK,
                                                     ae_max_entries=4, cmd_ppm=1_000_000, drop_ppm=50_000)

    def run(x):
        R = x.R
        x.step(60)
        st = x.read_state()
        rng = np.random.default_rng(17)

        def batch(g0, g1, kind):
            rows = []
            for g in range(g0, g1):
                for r in range(R):
                    last, term = int(fld(st, R, r, "last")[g]), int(fld(st, R, r, "term")[g])
                    if kind == "hs":
                        rows += _run_records(g, r, term + 1, -1, None, [])
                    elif kind == "tr":
                        rows += _run_records(g, r, term, r % R, min(g % 3, last), [])
                    else:
                        # r = 0: ENTRYs alone, standing on lastIndex; else a TRUNCATE 0 to 3 below it first
                        keep = None if r == 0 else max(0, last - (g + r) % 4)
                        at = last if keep is None else keep
                        ne = min(1 + (g + 2 * r) % 6, x.cap - at)
                        ent = [(at + j, term + (j > 1), int(rng.integers(0, 1 << 32))) for j in range(ne)]
                        rows += _run_records(g, r, term if r != 1 else None, -1, keep, ent)
            return WM.records(rows)

        infos = [x.replay(batch(0, 50, "whole"))]
        whole = batch(50, 70, "whole")
        infos += [x.replay(whole[k:k + 7]) for k in range(0, len(whole), 7)]
        infos.append(x.replay(batch(70, 100, "whole")))
        infos.append(x.replay(batch(100, 130, "tr")))
        infos.append(x.replay(batch(130, 160, "hs")))
        infos.append(x.replay(batch(160, 200, "whole"), keep_volatile=True))
        if not W:
            rows = _run_records(200, 2, 9, -1, 0, [(j, 1 + j // 100, 7000 + j) for j in range(580)])
            infos.append(x.replay(WM.records(rows)))
        x.step(20)
        tot = {k: sum(i[k] for i in infos) for k in infos[0]}
        return dict(tot, calls=len(infos))
    return dict(kw=kw, run=run)


def _scenarios():
    import restart_model as RM
    out = {}
    for mode, mname in ((abi.MODE_REFERENCE, "ref"), (abi.MODE_TEXTBOOK, "tb")):
        for R in (3, 5, 7):
            out[f"handlers-{mname}-R{R}-flat"] = handlers(R, mode, False, 10_000, 7 + R)
            out[f"handlers-{mname}-R{R}-ring"] = handlers(R, mode, True, 10_000, 647 + R)
        for n in (1, 65):
            out[f"handlers-{mname}-ragged-n{n}"] = handlers(5, mode, False, n, 41 + n, G=50)
        out[f"handlers-{mname}-skewed"] = handlers(5, mode, False, 6000, 29, G=300, skew=True)
        for ring in (False, True):
            out[f"consumer-{mname}-{'ring' if ring else 'flat'}"] = consumer(mode, ring)
            for kind in ("propose", "noops"):
                out[f"client-{kind}-{mname}-{'ring' if ring else 'flat'}"] = client(kind, mode, ring)
            out[f"outbox-{mname}-{'ring' if ring else 'flat'}"] = outbox("textbook" if mode else "reference",
                                                                         "ring" if ring else "flat")
        for kind in ("propose", "noops"):
            out[f"client-{kind}-{mname}-crafted"] = crafted_client(kind, mode)
    out.update(_step_scenarios())
    for variant in ("flat", "textbook", "ring"):
        for flags, fname in ((0, "persistent"), (RM.REPLAY, "replay"), (RM.AMNESIA, "amnesia")):
            out[f"restart-{variant}-{fname}"] = restarts(variant, flags)
    out["install-flat"], out["install-ring16"] = installs(False), installs(True)
    out["replay-flat"], out["replay-ring16"] = replays(False), replays(True)
    return out


SCENARIOS = _scenarios()
