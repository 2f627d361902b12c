"""The proposal outbox restated in plain Python on top of client_model.propose /
client_model.resolve (include/raft_engine.h, raft_engine_outbox_configure,
raft_outbox_submit, raft_engine_outbox_pump, raft_engine_outbox_read / write):
the reference of test_outbox_cpu.py (over the oracle alone) and
test_gpu_outbox.py (against the engine's kernels).  Nothing here touches a
device.

A pump, on the state the call finds.  Phase 1: every record's verdict from the
resolve record of its ticket (NEW, NO_LEADER and LOG_FULL tickets stored
nothing: NONE), first match of COMMITTED -> done; expire_steps > 0 and age >=
expire_steps -> done (EXPIRED); UNKNOWN -> keep; PENDING -> keep; LOST with
holders >= 1 -> keep (orphaned: another replica still holds the entry and may
yet commit it); LOST with holders == 0, or NONE -> retry.  Phase 2: the first
max_done done records leave in queue order, the retried ones are proposed with
one client_model.propose over their (group, cmd) in queue order, the queue
becomes the survivors in their original order."""
from __future__ import annotations

import functools

import numpy as np

import oracle as O
import client_model as CM
import noop_model as NM
import restart_model as RM
from helpers import STRESS_MIX, abi, blank_groups, fld, set_fld

NEW, DONE_COMMITTED, DONE_EXPIRED = abi.OUTBOX_NEW, abi.OUTBOX_COMMITTED, abi.OUTBOX_EXPIRED
ENTRY, DONE = abi.OUTBOX_ENTRY_DTYPE, abi.OUTBOX_DONE_DTYPE
V_PENDING, V_ORPHANED, V_UNKNOWN, V_RETRY, V_COMMITTED, V_EXPIRED = range(6)
INT32 = np.iinfo(np.int32)


class OutboxError(Exception):
    """A refused call of the model's Host: `code` is the RAFT_E* the engine returns."""

    def __init__(self, code: int, what: str = ""):
        super().__init__(f"{what} ({code})")
        self.code = code


def zero_info() -> dict:
    d = dict.fromkeys(abi.OUTBOX_INFO_FIELDS, 0)
    d["age_hist"] = [0] * 32
    return d


def bucket(age: int) -> int:
    return min(31, (max(age, 0) + 1).bit_length() - 1)


def entries(groups, cmds, tags, born: int) -> np.ndarray:
    """What a submit appends: status NEW, the ticket words (-1, -1, 0), tries 0."""
    q = np.zeros(len(groups), dtype=ENTRY)
    q["tag"], q["born"], q["group"], q["cmd"] = tags, born, groups, cmds
    q["replica"], q["index"], q["status"] = -1, -1, NEW
    return q


def verdicts(state, terms, logcmds, queue, now: int, expire: int, R: int, cap: int, W: int = 0, rule: str = "outbox"):
    """Phase 1: the verdict of every record.  rule "naive" is the wrong rule the
    outbox exists to replace: retry whatever resolved LOST."""
    tk = np.zeros(len(queue), dtype=abi.TICKET_DTYPE)
    for f in ("replica", "index", "term", "status"):
        tk[f] = queue[f]
    tk["status"][queue["status"] == NEW] = CM.NO_LEADER            # stored nothing: NONE
    rec, _ = CM.resolve(state, terms, logcmds, queue["group"].astype(np.int64), tk, queue["cmd"], R, cap, W)
    out = np.zeros(len(queue), np.uint8)
    for m in range(len(queue)):
        st, holders, age = int(rec["status"][m]), int(rec["holders"][m]), now - int(queue["born"][m])
        if st == CM.COMMITTED:
            v = V_COMMITTED
        elif expire > 0 and age >= expire:
            v = V_EXPIRED
        elif st == CM.UNKNOWN:
            v = V_UNKNOWN
        elif st == CM.PENDING:
            v = V_PENDING
        elif st == CM.LOST and holders >= 1 and rule == "outbox":
            v = V_ORPHANED
        else:
            assert st in (CM.LOST, CM.NONE), st
            v = V_RETRY
        out[m] = v
    return out


def pump(o, queue, now: int, expire: int, max_done: int, textbook: bool, W: int = 0, rule: str = "outbox"):
    """raft_engine_outbox_pump on the oracle `o`: (queue afterwards, done
    records, info, return code, verdicts)."""
    n = len(queue)
    info = zero_info()
    if n == 0:
        return queue, np.zeros(0, DONE), info, abi.RAFT_OK, np.zeros(0, np.uint8)
    v = verdicts(o.read_state(), *o.read_log(), queue, now, expire, o.R, o.cap, W, rule)
    fin = np.flatnonzero(v >= V_COMMITTED)
    out_idx, retry = fin[:max_done], np.flatnonzero(v == V_RETRY)
    done = np.zeros(len(out_idx), DONE)
    for k, m in enumerate(out_idx):
        age = int(np.clip(now - int(queue["born"][m]), INT32.min, INT32.max))
        com = v[m] == V_COMMITTED
        done[k] = (queue["tag"][m], queue["group"][m], DONE_COMMITTED if com else DONE_EXPIRED, queue["index"][m],
                   queue["term"][m], queue["tries"][m], age)
        if com:
            info["age_hist"][bucket(age)] += 1
            info["committed"] += 1
        else:
            info["expired"] += 1
    queue = queue.copy()
    prc = abi.RAFT_OK
    if len(retry):
        tk, prc = CM.propose(o, queue["group"][retry].astype(np.int64), queue["cmd"][retry], textbook, W)
        for f in ("replica", "index", "term", "status"):
            queue[f][retry] = tk[f]
        queue["tries"][retry] += 1
        for name, code in (("accepted", CM.ACCEPTED), ("ghosted", CM.GHOSTED), ("no_leader", CM.NO_LEADER),
                           ("log_full", CM.LOG_FULL)):
            info[name] = int((tk["status"] == code).sum())
    keep = np.ones(n, bool)
    keep[out_idx] = False
    info.update(queued=n, deferred=len(fin) - len(out_idx), pending=int((v == V_PENDING).sum()),
                orphaned=int((v == V_ORPHANED).sum()), unknown=int((v == V_UNKNOWN).sum()), retried=len(retry),
                left=int(keep.sum()))
    rc = abi.RAFT_EWINDOW if info["unknown"] or prc == abi.RAFT_EWINDOW else abi.RAFT_OK
    return queue[keep], done, info, rc, v


def check_entries(q: np.ndarray, G: int, R: int, cap: int):
    """raft_engine_outbox_write's refusals; None when every record is acceptable."""
    if ((q["group"] < 0) | (q["group"] >= G)).any():
        return abi.RAFT_ERANGE
    known = (q["status"] == NEW) | ((q["status"] >= CM.ACCEPTED) & (q["status"] <= abi.PROPOSE_CURRENT))
    stored = known & (q["status"] != NEW) & (q["status"] != CM.NO_LEADER) & (q["status"] != CM.LOG_FULL)
    bad = ~known | (q["tries"] < 0) | (q["pad"] != 0) | (stored & ((q["replica"] < -1) | (q["replica"] >= R) |
                                                                    (q["index"] < 0) | (q["index"] >= cap)))
    return abi.RAFT_EINVAL if bad.any() else None


class Host(NM.Host):
    """noop_model's Host (the oracle under RaftEngine's method names) with the
    outbox.  `rule` "naive" swaps in the retry-every-LOST rule.  `seen_orphaned`
    collects the tags a pump counted as orphaned."""

    def __init__(self, slots: int = 0, rule: str = "outbox", **kw):
        super().__init__(slots, **kw)
        self.rule = rule
        self.ob_cap = None
        self.seen_orphaned = set()

    def reset(self):
        """raft_engine_reset: the groups as created at step 0, an empty outbox."""
        self.o.close()
        self.o = O.Oracle(self.p)
        if self.ob_cap is not None:
            self.queue = np.zeros(0, ENTRY)

    def outbox_configure(self, capacity: int, expire_steps: int = 0):
        if capacity < 1 or expire_steps < 0 or (self.ob_cap is not None and len(self.queue)):
            raise OutboxError(abi.RAFT_EINVAL, "outbox_configure")
        self.ob_cap, self.ob_expire, self.queue = capacity, expire_steps, np.zeros(0, ENTRY)

    def _configured(self, what):
        if self.ob_cap is None:
            raise OutboxError(abi.RAFT_EINVAL, what)

    def outbox_submit(self, groups, cmds, tags):
        self._configured("outbox_submit")
        groups = np.asarray(groups, dtype=np.int64)
        if len(groups) > self.ob_cap - len(self.queue):
            raise OutboxError(abi.RAFT_EFULL, "outbox_submit")
        if len(groups) and (groups.min() < 0 or groups.max() >= self.G):
            raise OutboxError(abi.RAFT_ERANGE, "outbox_submit")
        self.queue = np.concatenate([self.queue, entries(groups, cmds, tags, self.step_index)])

    def outbox_len(self) -> int:
        self._configured("outbox_read")
        return len(self.queue)

    def outbox_pump(self, max_done=None):
        self._configured("outbox_pump")
        max_done = len(self.queue) if max_done is None else max_done
        before = self.queue
        self.queue, done, info, self.last_status, v = pump(self.o, self.queue, self.step_index, self.ob_expire, max_done,
                                                           self.textbook, self.W, self.rule)
        self.seen_orphaned.update(before["tag"][v == V_ORPHANED].tolist())
        return info, done

    def outbox_read(self) -> np.ndarray:
        self._configured("outbox_read")
        return self.queue.copy()

    def outbox_write(self, records):
        self._configured("outbox_write")
        if len(records) > self.ob_cap:
            raise OutboxError(abi.RAFT_EFULL, "outbox_write")
        code = check_entries(records, self.G, self.R, self.cap)
        if code is not None:
            raise OutboxError(code, "outbox_write")
        self.queue = np.array(records, dtype=ENTRY)


# ---- crafted groups: one per verdict, written with write_state / write_log ----
CR, CG, CCAP, CNOW, CEXPIRE = 3, 8, 16, 100, 50
CRAFTED_NAMES = ["committed", "pending", "orphaned", "gone", "no_leader", "log_full", "expired", "two_retries"]


def crafted():
    """(state, terms, cmds) of 8 groups of 3 replicas, log_cap 16.  Unless said
    otherwise every replica is in term 4 and holds 5 entries (term 1 + j // 2,
    cmd 1000 g + j, the same on all three), 3 of them committed, and replica 1
    leads:
      orphaned   replica 0's slot 4 was overwritten by a higher term (4, 7777);
                 replicas 1 and 2 still hold (4: term 3, cmd 2004)
      no_leader  nobody leads
      log_full   the leader's lastIndex = physLen = log_cap"""
    R, G, cap = CR, CG, CCAP
    w = blank_groups(G, R)
    t = np.zeros((G, R, cap), np.int32)
    c = np.zeros((G, R, cap), np.uint32)
    for g in range(G):
        t[g, :] = 1 + np.arange(cap) // 2
        c[g, :] = 1000 * g + np.arange(cap)
    for r in range(R):
        set_fld(w, R, r, "term", 4)
        set_fld(w, R, r, "last", 5)
        set_fld(w, R, r, "phys", 5)
        set_fld(w, R, r, "commit", 3)
    set_fld(w, R, 1, "role", abi.LEADER)
    t[2, 0, 4], c[2, 0, 4] = 4, 7777
    set_fld(w[4:5], R, 1, "role", abi.FOLLOWER)
    set_fld(w[5:6], R, 1, "last", cap)
    set_fld(w[5:6], R, 1, "phys", cap)
    return w, t, c


def _rec(tag, born, group, cmd, ticket, tries=0):
    return (tag, born, group, cmd, *ticket, tries, 0)


A = CM.ACCEPTED
NEW_TK = (-1, -1, 0, NEW)
# the queue written into the crafted engine at step index CNOW with expire_steps CEXPIRE, done / retry / keep interleaved
CRAFTED_QUEUE = np.array([
    _rec(10, 95, 0, 2, (1, 2, 2, A)),            # committed: index 2 < commitIndex 3
    _rec(11, 95, 3, 9999, (1, 4, 3, A)),         # gone: no replica holds (4: 3, 9999)
    _rec(12, 95, 1, 1004, (1, 4, 3, A), 2),      # pending: on its own replica, not committed
    _rec(13, 95, 7, 501, NEW_TK),                # two_retries, first
    _rec(14, 10, 6, 6004, (1, 4, 3, A)),         # expired: pending, but 90 steps old
    _rec(15, 95, 2, 2004, (0, 4, 3, A)),         # orphaned: LOST on replica 0, held by two others
    _rec(16, 95, 4, 502, NEW_TK),                # no_leader
    _rec(17, 95, 7, 503, NEW_TK),                # two_retries, second: the next index
    _rec(18, 95, 5, 504, NEW_TK),                # log_full
    _rec(19, 95, 0, 1, (1, 1, 1, A)),            # committed, behind everything else in the queue
], dtype=ENTRY)
# ... and what a pump with room for everything must leave and hand out, written out by hand
CRAFTED_DONE = np.array([(10, 0, DONE_COMMITTED, 2, 2, 0, 5), (14, 6, DONE_EXPIRED, 4, 3, 0, 90),
                         (19, 0, DONE_COMMITTED, 1, 1, 0, 5)], dtype=DONE)
CRAFTED_LEFT = np.array([
    _rec(11, 95, 3, 9999, (1, 5, 4, A), 1),
    _rec(12, 95, 1, 1004, (1, 4, 3, A), 2),
    _rec(13, 95, 7, 501, (1, 5, 4, A), 1),
    _rec(15, 95, 2, 2004, (0, 4, 3, A)),
    _rec(16, 95, 4, 502, (-1, -1, 0, CM.NO_LEADER), 1),
    _rec(17, 95, 7, 503, (1, 6, 4, A), 1),
    _rec(18, 95, 5, 504, (1, CCAP, 4, CM.LOG_FULL), 1),
], dtype=ENTRY)
CRAFTED_INFO = dict(zero_info(), queued=10, committed=2, expired=1, deferred=0, pending=1, orphaned=1, unknown=0,
                    retried=5, accepted=3, ghosted=0, no_leader=1, log_full=1, left=7,
                    age_hist=[0, 0, 2] + [0] * 29)


def crafted_cut(max_done: int):
    """(done, queue afterwards, info) of the crafted pump cut at max_done < 3:
    the done records past the cut stay where they were, unchanged."""
    done = CRAFTED_DONE[:max_done]
    stay = {int(t): CRAFTED_QUEUE[CRAFTED_QUEUE["tag"] == t][0] for t in CRAFTED_DONE["tag"][max_done:]}
    after = {int(r["tag"]): r for r in CRAFTED_LEFT}
    after.update(stay)
    left = np.array([after[int(t)] for t in CRAFTED_QUEUE["tag"] if int(t) in after], dtype=ENTRY)
    com = int((done["status"] == DONE_COMMITTED).sum())
    info = dict(CRAFTED_INFO, committed=com, expired=len(done) - com, deferred=3 - max_done, left=7 + 3 - max_done,
                age_hist=[0, 0, com] + [0] * 29)
    return done, left, info


def crafted_host(textbook: bool, **more) -> Host:
    kw = dict(R=CR, G=CG, log_cap=CCAP, **(dict(mode=abi.MODE_TEXTBOOK) if textbook else {}))
    h = Host(**kw, **more)
    load_crafted(h)
    return h


def load_crafted(x):
    """The crafted state, step index and queue into `x` (a Host or a RaftEngine)."""
    w, t, c = crafted()
    x.write_state(w) if hasattr(x, "write_state") else x.o.write_state(w)
    x.write_log(t, c) if hasattr(x, "write_log") else x.o.write_log(t, c)
    if hasattr(x, "o"):
        x.o.step_index = CNOW
    else:
        x.step_index = CNOW
    x.outbox_configure(32, CEXPIRE)
    x.outbox_write(CRAFTED_QUEUE)


# below a 16-slot window: one group whose replicas hold 40 entries; a ticket for index 3 cannot be judged
RING_W, RING_CAP = 16, 64
RING_QUEUE = np.array([_rec(30, 0, 0, 77, (1, 3, 2, A)), _rec(31, 0, 0, 78, (1, 39, 2, A))], dtype=ENTRY)


def crafted_ring():
    R = CR
    w = blank_groups(1, R)
    t = np.full((1, R, RING_CAP), 2, np.int32)
    c = np.zeros((1, R, RING_CAP), np.uint32)
    c[0, :, 39] = 78
    for r in range(R):
        set_fld(w, R, r, "term", 3)
        set_fld(w, R, r, "last", 40)
        set_fld(w, R, r, "phys", 40)
        set_fld(w, R, r, "commit", 30)
    set_fld(w, R, 1, "role", abi.LEADER)
    return w, t, c


RING_KW = dict(R=CR, G=1, log_cap=RING_CAP, log_window=RING_W, mode=abi.MODE_TEXTBOOK)
RING_INFO = dict(zero_info(), queued=2, pending=1, unknown=1, left=2)


# ---- the parity scenario shared by test_outbox_cpu.py (non-vacuity, on the
# oracle alone) and test_gpu_outbox.py (the engine against it)
PARITY_R = (1, 3, 5, 8)
PARITY_G = 203
PARITY_CASES = [(R, mode, log) for R in PARITY_R for mode in ("reference", "textbook") for log in ("flat", "ring")]
SIZES = (1, 63, 64, 65, 700)
PARITY_ROUNDS = 10


def parity_kw(R: int, mode: str, log: str) -> dict:
    return dict(R=R, G=PARITY_G, seed=11, log_cap=300, **STRESS_MIX,
                **(dict(mode=abi.MODE_TEXTBOOK, ae_max_entries=4) if mode == "textbook" else {}),
                **(dict(log_window=16) if log == "ring" else {}))


def batch_of(rng, size: int, G: int, k: int):
    """Batch k: uniformly random groups, the hot group's burst of 24 in a batch
    of 700 (client_model.batch_of); commands and tags distinct over the run."""
    groups = rng.integers(0, G, size, dtype=np.int64)
    if size == 700:
        groups[rng.choice(size, 24, replace=False)] = (37 * k + 11) % G
    base = 1_000_000 * (k + 1)
    return groups, (base + np.arange(size)).astype(np.uint32), base + np.arange(size, dtype=np.int64)


def parity_run(x, label: str = "", outbox: bool = True) -> list:
    """The scenario on `x` (a Host or a RaftEngine): 10 steps, configure, a pump
    of the empty queue, then ten rounds of 5 steps, a submit, a pump (every
    third one cut at 5 done records), no-ops where a pump left only PENDING
    records, and a persistent restart after rounds 3 and 7.  With outbox False
    the same steps and restarts without any outbox call.  Returns the
    checkpoints, each a dict of everything that must be equal between the
    engine and the oracle."""
    out = []

    def snap(what, **more):
        out.append(dict(what=f"{label} {what}", state=x.read_state(), logs=x.read_log(), digest=x.digest(), **more))

    rng = np.random.default_rng(7)
    snap("warm-up", counters=x.step(10))
    if outbox:
        x.outbox_configure(4096, 40)
        info, done = x.outbox_pump()
        snap("empty pump", info=info, done=done, rc=x.last_status, queue=x.outbox_read())
    for k in range(PARITY_ROUNDS):
        snap(f"round {k}", counters=x.step(5))
        groups, cmds, tags = batch_of(rng, SIZES[k % len(SIZES)], x.G, k)
        if outbox:
            x.outbox_submit(groups, cmds, tags)
            info, done = x.outbox_pump(5 if k % 3 == 2 else None)
            snap(f"pump {k}", info=info, done=done, rc=x.last_status, queue=x.outbox_read())
            if info["left"] and info["left"] == info["pending"]:
                snap(f"noops {k}", noops=x.append_noops(cmd=NM.NOOP))
        if k in (3, 7):
            snap(f"restart {k}", restart=x.restart(ppm=150_000))
    snap("run-on", counters=x.step(10))
    return out


@functools.lru_cache(maxsize=None)
def host_parity_run(R: int, mode: str, log: str):
    """parity_run on the oracle, once per input and shared.  Treat it as read-only."""
    h = Host(**parity_kw(R, mode, log))
    points = parity_run(h, f"R{R} {mode} {log}")
    h.close()
    return points


def totals(points) -> dict:
    """The pump infos of a run summed: the non-vacuity conditions."""
    tot = zero_info()
    for p in points:
        if "info" in p:
            for k in abi.OUTBOX_INFO_FIELDS:
                tot[k] += p["info"][k]
    return tot


def assert_same_points(got: list, want: list, R: int, upto=None):
    """Every checkpoint of the engine's parity_run equals the oracle's, bit for
    bit, as long as the run is valid: on a ring, up to the first step in which
    the oracle counts a window miss (restart_model.assert_same_rows) or the
    first pump whose retried add was below a window."""
    from helpers import assert_same_logs, assert_same_state
    assert len(got) == len(want)
    for a, b in list(zip(got, want))[:upto]:
        label = b["what"]
        if "counters" in b and not RM.assert_same_rows(a["counters"], b["counters"], label):
            return
        for k in ("done", "queue"):
            if k in b:
                assert a[k].dtype == b[k].dtype and len(a[k]) == len(b[k]), f"{label}: {k} {len(a[k])} vs {len(b[k])}"
                if not np.array_equal(a[k], b[k]):
                    at = int(np.flatnonzero(a[k] != b[k])[0])
                    raise AssertionError(f"{label}: {k} differ first at {at}: {a[k][at]} vs {b[k][at]}")
        for k in ("info", "rc", "noops", "restart"):
            assert a.get(k) == b.get(k), f"{label}: {k} {a.get(k)} vs {b.get(k)}"
        if b.get("rc") == abi.RAFT_EWINDOW and not b["info"]["unknown"]:
            return
        assert_same_state(a["state"], b["state"], R, label)
        assert_same_logs(a["state"], a["logs"], b["logs"], R, label)
        assert a["digest"] == b["digest"], f"{label}: digest differs with equal state and logs"


def first_retry(points) -> int:
    """The index of the first checkpoint whose pump retried something."""
    return next(i for i, p in enumerate(points) if p.get("info", {}).get("retried"))


# ---- the property: textbook mode, persistent restarts, commands committed once ----
PROPERTY_KW = dict(R=5, G=203, seed=11, log_cap=300, mode=abi.MODE_TEXTBOOK, ae_max_entries=4,
                   **dict(STRESS_MIX, cmd_ppm=0))
PROPERTY_STEPS, PROPERTY_BATCH = 300, 40
# the seed of the property run (the engine's and the submits'): of seeds 1.. the first on which the naive rule
# commits a command twice; under the outbox's rule the same run has two orphans that commit later
ORPHAN_SEED = 13


def committed_places(state, terms, cmds, R: int, cap: int) -> dict:
    """(group, cmd) -> the set of (index, term) under which some replica's committed prefix holds cmd."""
    out = {}
    for g in range(state.shape[0]):
        for r in range(R):
            hi = int(np.clip(min(fld(state, R, r, "commit")[g], fld(state, R, r, "last")[g]), 0, cap))
            for i in range(hi):
                out.setdefault((g, int(cmds[g, r, i])), set()).add((i, int(terms[g, r, i])))
    return out


@functools.lru_cache(maxsize=None)
def property_run(seed: int, rule: str = "outbox", steps: int = PROPERTY_STEPS):
    """The stress mix with a persistent restart_random every 20 steps, a submit
    of PROPERTY_BATCH distinct commands and a pump every 5 steps, no-ops where a
    pump left only PENDING records; at the end no more submits, and pumps until
    the queue is empty or 100 more steps passed.  Returns a dict: completions
    (every done record), cmd_of (tag -> (group, cmd)), queued (tags still in the
    queue), places (committed_places of the final state), orphaned (tags a pump
    counted as orphaned), totals."""
    h = Host(rule=rule, **dict(PROPERTY_KW, seed=seed))
    h.outbox_configure(1 << 16, 0)
    rng = np.random.default_rng(seed)
    cmd_of, done_all, tot, next_cmd = {}, [], zero_info(), 1

    def pump_once():
        info, done = h.outbox_pump()
        done_all.append(done)
        for k in abi.OUTBOX_INFO_FIELDS:
            tot[k] += info[k]
        if info["left"] and info["left"] == info["pending"]:
            h.append_noops(cmd=NM.NOOP)
        return info

    t = 0
    while t < steps:
        h.step(5)
        t += 5
        if t % 20 == 0:
            h.restart(ppm=100_000)
        groups = rng.integers(0, h.G, PROPERTY_BATCH, dtype=np.int64)
        cmds = (next_cmd + np.arange(PROPERTY_BATCH)).astype(np.uint32)
        next_cmd += PROPERTY_BATCH
        h.outbox_submit(groups, cmds, cmds.astype(np.int64))
        cmd_of.update({int(c): (int(g), int(c)) for g, c in zip(groups, cmds)})
        pump_once()
    for _ in range(20):
        h.step(5)
        if pump_once()["left"] == 0:
            break
    st, (terms, cmds) = h.read_state(), h.read_log()
    out = dict(completions=np.concatenate(done_all), cmd_of=cmd_of, queued=h.outbox_read()["tag"].tolist(),
               places=committed_places(st, terms, cmds, h.R, h.cap), orphaned=set(h.seen_orphaned), totals=tot)
    h.close()
    return out


def duplicates(run: dict) -> list:
    """The submitted commands a run committed under more than one (index, term)."""
    return [k for k in run["cmd_of"].values() if len(run["places"].get(k, ())) > 1]
