"""RaftService — the reference's per-node API over the batched engine.

The reference node is ``class RaftServer(val id: Int, val servers: List<RaftClient>)``
(RaftServer.kt:28) serving ``service Raft { Vote; Append }`` (greeter.proto:46-49)
plus ``appendCommand`` / ``entries`` (RaftServer.kt:96-107).  Here a node is one
(group, replica) slot of a RaftEngine; ``RaftNode`` has the same method names,
argument meaning and error behaviour:

* ``vote(RequestVoteRPC) -> ResponseVoteRPC``           (RaftServer.kt:228-251)
* ``append(RequestAppendEntriesRPC) -> ResponseAppendEntriesRPC``
  (RaftServer.kt:253-287); raises ``IndexError`` where the reference's
  ``Log.get`` throws (prevLogIndex < -1), after the handler's earlier effects
* ``appendCommand(command: str) -> str``                 (RaftServer.kt:100-107)
* ``entries() -> list[str]`` in the reference's ``"term: command"`` format
  (RaftServer.kt:96-97)
* ``lastApplied`` (RaftServer.kt:47) and ``RaftService.poll_committed``: the
  entries that became committed since the last poll, for a state machine to apply
* ``RaftService.apply_committed`` / ``read`` and ``RaftNode.machine``: the
  replicated state machine on the device -- committed entries applied where
  they are, a register read routed to the leader, a node's head and registers
* ``RaftService.read_linearizable``: the read a client can trust -- a ReadIndex
  ticket from the group's newest leader, confirmed against a majority of the
  group's terms before the register is read
* ``RaftService.transfer_leadership`` / ``drain_node`` and ``RaftNode.step_down``:
  leadership moved on purpose (Raft thesis §3.10; the reference's leader only
  loses it by timeout) -- one group's, or every group a node leads before a
  planned restart of that node
* ``RaftService.assert_leadership``: a new leader's no-op entry (Raft thesis
  §3.6.2), so that an idle group commits what earlier terms left and serves
  linearizable reads; ``entries()`` shows it as ``RaftService.NOOP_COMMAND``
* ``RaftService.watch_leaders`` / ``newest_leader``: a leader directory kept
  up to date from the engine's leader watch -- only the groups whose leader or
  term changed since the last call cross the bus (etcd's SoftState in a Ready)
* ``RaftService.submit_reliable`` / ``completions`` / ``pump_until_idle``: the
  engine's proposal outbox -- commands held on the device until committed,
  re-proposed only when no replica holds them any more, completed once
* ``RaftService.check_safety`` / ``violations``: the engine's safety audit --
  Raft's invariants checked over time on the device, and the groups that
  broke one, with the step at which it was first seen
* ``RaftService.check_liveness`` / ``unavailable`` / ``remediate``: the engine's
  liveness monitor -- which groups have no leader, a stalled commit or a
  lagging replica now and since when, and the no-ops and snapshot installs
  aimed at exactly those
* ``RaftService.persist`` / ``recover``: the engine's persistence stream -- the
  hard state and the log entries that changed since the last call, applied to
  a host-side image of every node's disk (etcd's HardState and Entries in a
  Ready), and a node given back what it had persisted after it lost it;
  ``recover_on_device`` does that for many nodes in one device call (the
  engine's WAL replay) and ``standby`` keeps a second engine in step from it
* ``RaftService.leader`` / ``submit`` / ``status``: what a client of the
  reference's ``/cmd/{command}`` route (RaftServer.kt:87-88) needs -- the group's
  leader, a command routed to it with a ticket, and that ticket's fate

Commands are strings in the reference (LogEntry.command, greeter.proto:31); the
engine stores a u32 id per entry, interned here.  Every call is one HIP batch;
``RaftService.vote_many`` / ``append_many`` batch many nodes per launch.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

from . import abi, replay, wire
from .engine import RaftEngine, WalImage


@dataclass
class LogEntry:                        # RequestAppendEntriesRPC.LogEntry, greeter.proto:29-32
    term: int
    command: str


@dataclass
class RequestVoteRPC:                  # greeter.proto:16-21
    term: int
    candidateId: int
    lastLogIndex: int
    lastLogTerm: int


@dataclass
class ResponseVoteRPC:                 # greeter.proto:23-26
    term: int
    voteGranted: bool


@dataclass
class RequestAppendEntriesRPC:         # greeter.proto:28-39
    term: int
    leaderId: int
    prevLogIndex: int
    prevLogTerm: int
    entries: List[LogEntry] = field(default_factory=list)
    leaderCommit: int = 0


@dataclass
class ResponseAppendEntriesRPC:        # greeter.proto:41-44
    term: int
    success: bool


class CommandTable:
    """Interns LogEntry.command strings to the engine's u32 command ids."""

    BASE = 0x80000000

    def __init__(self):
        self._ids: dict[str, int] = {}
        self._names: dict[int, str] = {}

    def intern(self, s: str) -> int:
        i = self._ids.get(s)
        if i is None:
            i = self.BASE + len(self._ids)
            if i > 0xFFFFFFFF:
                raise OverflowError("command table full")
            self._ids[s] = i
            self._names[i] = s
        return i

    def lookup(self, s: str) -> Optional[int]:
        """The id of a string interned before, or None: never grows the table."""
        return self._ids.get(s)

    def name(self, i: int) -> str:
        # commands injected by the lockstep harness carry Philox ids
        return self._names.get(int(i), f"cmd#{int(i):08x}")


class RaftNode:
    """One reference RaftServer: replica ``replica`` (id = replica + 1) of ``group``."""

    def __init__(self, service: "RaftService", group: int, replica: int):
        self.s = service
        self.group = group
        self.replica = replica
        self.id = replica + 1

    # -- RaftGrpcKt.RaftImplBase overrides ---------------------------------
    def vote(self, request: RequestVoteRPC) -> ResponseVoteRPC:
        return self.s.vote_many([self.group], [self.replica], [request])[0]

    def append(self, request: RequestAppendEntriesRPC) -> ResponseAppendEntriesRPC:
        return self.s.append_many([self.group], [self.replica], [request])[0]

    def appendCommand(self, command: str) -> str:      # RaftServer.kt:100-107
        self.s.engine.append_command_batch([self.group], [self.replica], [self.s.commands.intern(command)])
        return command

    def entries(self) -> List[str]:                      # RaftServer.kt:96-97
        return [f"{t}: {c}" for t, c in self.log()]

    # -- inspection ----------------------------------------------------------
    def log(self) -> List[tuple]:
        """Visible entries log[0 .. lastIndex) as (term, command) (Commons.kt:71-72)."""
        st = self._fields()
        terms, cmds = self.s.engine.read_log(self.group, 1)
        n = int(st[abi.F_INDEX["last"]])
        return [(int(terms[0, self.replica, j]), self.s.commands.name(cmds[0, self.replica, j])) for j in range(n)]

    def _fields(self) -> np.ndarray:
        w = self.s.engine.read_state(self.group, 1)[0]
        return w[self.replica * abi.NUM_FIELDS:(self.replica + 1) * abi.NUM_FIELDS]

    @property
    def currentTerm(self) -> int:
        return int(self._fields()[abi.F_INDEX["term"]])

    @property
    def votedFor(self) -> int:
        return int(self._fields()[abi.F_INDEX["voted"]])

    @property
    def state(self) -> str:
        return ("FOLLOWER", "CANDIDATE", "LEADER")[int(self._fields()[abi.F_INDEX["role"]])]

    @property
    def commitIndex(self) -> int:
        return int(self._fields()[abi.F_INDEX["commit"]])

    @property
    def lastApplied(self) -> int:                         # RaftServer.kt:47 (declared there, never used)
        """Entries [0, lastApplied) of this node's log were handed out by poll_committed."""
        return int(self.s.engine.applied(self.group, 1)[0, self.replica])

    def restart(self, amnesia: bool = False, replay: bool = False, down_steps: int = 0) -> dict:
        """Kill this node's process and launch it again (main, RaftServer.kt:302-310).
        amnesia=True is what the reference does, since it persists nothing:
        entries() is empty and currentTerm is 0 afterwards.  down_steps cuts
        the restarted node off for that long; to cut a node off WITHOUT
        restarting it (its state kept, its timers running) use isolate()."""
        return self.s.restart([self.group], [self.replica], amnesia=amnesia, replay=replay, down_steps=down_steps)

    def isolate(self, steps: int, replace: bool = False) -> str:
        """Unplug this node's network cable for `steps` (RaftService.isolate):
        nothing it sends arrives and nothing reaches it, its state stays and
        its timers run -- a leader goes on calling itself LEADER.  Returns the
        ticket's status name ("SET", or "BUSY" when another isolation of the
        group is running and replace is False)."""
        tk = self.s.isolate([self.group], [self.replica], steps, replace=replace)
        return abi.ISOLATE_STATUS_NAMES[int(tk["status"][0])]

    def install(self, min_lag: int = 0) -> dict:
        """Bring this node up to its group's newest leader (RaftEngine.install_snapshot
        with only this node eligible): the leader's retained log, commit point
        and machine.  Nothing happens to the leader itself, to a node in a
        higher term, or in a group without a leader; the info says which."""
        return self.s.engine.install_snapshot(np.array([1 << self.replica], dtype=np.uint8), g0=self.group,
                                              min_lag=min_lag)

    def step_down(self) -> str:
        """Hand this node's leadership on to the best-placed other node of its
        group (RaftService.transfer_leadership).  Returns the ticket's status
        name: "SENT", or why nothing was sent; "NOT_LEADER", before any write,
        when this node is not its group's newest leader."""
        w = self.s.engine.read_state(self.group, 1)[0].reshape(-1)[:self.s.engine.R * abi.NUM_FIELDS]
        w = w.reshape(self.s.engine.R, abi.NUM_FIELDS)
        lead = [(-int(t), r) for r, (t, role) in enumerate(zip(w[:, abi.F_INDEX["term"]], w[:, abi.F_INDEX["role"]]))
                if role == abi.LEADER]
        if not lead or min(lead)[1] != self.replica:
            return "NOT_LEADER"
        return self.s.transfer_leadership(self.group)

    def machine(self) -> tuple:
        """This node's state machine: (head, registers) -- head a record of
        abi.SM_HEAD_DTYPE (applied, lost, hash), registers [slots] uint32."""
        h, r = self.s.engine.sm_read(self.group, 1)
        return h[0, self.replica], r[0, self.replica]


class RaftService:
    """The `service Raft` surface of every node of a RaftEngine."""

    def __init__(self, engine: RaftEngine):
        self.engine = engine
        self.commands = CommandTable()

    def node(self, group: int, replica: int) -> RaftNode:
        if not (0 <= group < self.engine.G and 0 <= replica < self.engine.R):
            raise IndexError((group, replica))
        return RaftNode(self, group, replica)

    def vote_many(self, groups, replicas, requests: List[RequestVoteRPC]) -> List[ResponseVoteRPC]:
        q = np.array([[r.term, r.candidateId, r.lastLogIndex, r.lastLogTerm] for r in requests],
                     dtype=np.int32).reshape(-1, 4)
        out = self.engine.vote_batch(groups, replicas, q)
        return [ResponseVoteRPC(int(t), bool(g)) for t, g in out]

    def append_many(self, groups, replicas, requests: List[RequestAppendEntriesRPC]) -> List[ResponseAppendEntriesRPC]:
        rows = []
        for r in requests:
            # the reference appends only entries[0] (RaftServer.kt:278)
            e = r.entries[0] if r.entries else None
            rows.append([r.term, r.leaderId, r.prevLogIndex, r.prevLogTerm, int(e is not None),
                         e.term if e else 0, self.commands.intern(e.command) if e else 0, r.leaderCommit])
        out = self.engine.append_batch(groups, replicas, np.array(rows, dtype=np.int64).reshape(-1, 8))
        res = []
        for t, s, status in out:
            if status != 0:
                raise IndexError("Log.get: prevLogIndex out of bounds (RaftServer.kt:276, Commons.kt:53-54)")
            res.append(ResponseAppendEntriesRPC(int(t), bool(s)))
        return res

    def poll_committed(self, g0: int = 0, n: Optional[int] = None, replica: int = -1,
                       max_entries: Optional[int] = None):
        """The apply loop's input: yields (group, replica, index, term, command)
        for every entry of groups [g0, g0 + n) that became committed since the
        last poll, in ascending (group, replica, index) order, and advances
        lastApplied past them (one drain_committed call: no whole-log copy).
        ``last_poll`` keeps that call's info (pending, lost, regressed)."""
        # the drain runs now, not at the first next(): the returned iterator only decodes
        rec, self.last_poll = self.engine.drain_committed(g0, n, replica, max_entries)
        name = self.commands.name
        return ((g, r, i, t, name(c)) for g, r, i, t, c in
                zip(rec["group"].tolist(), rec["replica"].tolist(), rec["index"].tolist(), rec["term"].tolist(),
                    rec["cmd"].tolist()))

    # -- the replicated state machine: committed entries applied on the device ---
    def apply_committed(self, g0: int = 0, n: Optional[int] = None, replica: int = -1) -> dict:
        """Apply every entry of groups [g0, g0 + n) that became committed since
        the machines' cursors (engine.sm_configure first): one kernel, no copy to
        the host.  Returns the info (applied, lost, regressed, status).  A string
        command lands in the register its interned id's low bits name."""
        return self.engine.sm_apply(g0, n, replica)

    def read(self, groups, keys: List[str], replica=-1) -> List[tuple]:
        """The client's read: per request (command, replica, applied, commit) --
        the command last applied to the register that keys[m] maps to (its
        interned id's low bits; named by CommandTable.name), on `replica` of
        groups[m] (-1: the group's leader; replica -1 back: it has none), with
        that replica's applied cursor and commitIndex.  A read changes nothing:
        a key that was never interned has no id, hence no register; it raises
        KeyError before any device call."""
        ids = [self.commands.lookup(k) for k in keys]
        unknown = [k for k, i in zip(keys, ids) if i is None]
        if unknown:
            raise KeyError(f"read: never submitted, so no register holds it: {unknown[0]!r}")
        v = self.engine.sm_get(groups, ids, replica)
        name = self.commands.name
        return [(name(c), r, a, m) for c, r, a, m in
                zip(v["value"].tolist(), v["replica"].tolist(), v["applied"].tolist(), v["commit"].tolist())]

    # -- leader no-op entries (Raft thesis §3.6.2; the reference has none) -------------------
    NOOP_COMMAND = "raft:noop"          # the reserved command string of a leader's no-op entry

    def assert_leadership(self, g0: int = 0, n: Optional[int] = None) -> dict:
        """Give every leader of groups [g0, g0 + n) that has no entry of its own
        term at the end of its log a no-op entry (RaftEngine.append_noops), so
        that it can commit what earlier terms left behind and serve
        linearizable reads after the next steps.  The entry's command is
        NOOP_COMMAND, interned on first use (a service that never calls this
        keeps its command ids); RaftNode.entries() and poll_committed show it
        under that name, and a configured machine passes over it.  Returns the
        info; ``last_noops`` keeps (groups, tickets, cmds) for RaftEngine.resolve."""
        e = self.engine
        cmd = self.commands.intern(self.NOOP_COMMAND)
        if e.sm_slots:
            e.sm_set_noop(cmd)
        info, tk, cmds = e.append_noops(g0, n, cmd, tickets=True)
        self.last_noops = (np.arange(g0, g0 + len(tk), dtype=np.int64), tk, cmds)
        return info

    def read_linearizable(self, groups, keys: List[str], assert_leadership: bool = False) -> List[tuple]:
        """The read a client can trust: per request (command, status name).
        One begin (a ReadIndex ticket from each group's newest leader), one
        serve of the tickets that were ISSUED (the leader confirmed against a
        majority of the group's terms), and where a leader's machine was BEHIND
        its read index an apply_committed of those groups alone (one call per
        run of consecutive group ids) and one more serve of them.  The engine is never stepped.  command is the one last applied
        to the register keys[m] maps to (named by CommandTable.name) when the
        status is "SERVED", else None; the other statuses are "BEHIND" (still,
        after the apply), "GAPPED", "NO_QUORUM", "DEPOSED", or why no ticket was
        issued: "NO_LEADER", "TERM_UNCOMMITTED", "UNKNOWN" -- the client retries
        after a step.  With assert_leadership=True the groups that answered
        "TERM_UNCOMMITTED" are given their leader's no-op entry
        (assert_leadership, one call per run of consecutive group ids) before
        the call returns, so that the retry after the next steps is ISSUED; off,
        the default, nothing is ever written.  ``last_read`` keeps (tickets,
        records).  Keys as in read: one that was never interned raises KeyError
        before any device call."""
        ids = [self.commands.lookup(k) for k in keys]
        unknown = [k for k, i in zip(keys, ids) if i is None]
        if unknown:
            raise KeyError(f"read_linearizable: never submitted, so no register holds it: {unknown[0]!r}")
        g = np.ascontiguousarray(groups, dtype=np.int64)
        k = np.asarray(ids, dtype=np.uint32)
        tk = self.engine.begin_reads(g)
        rec = np.zeros(len(g), dtype=abi.READ_RESULT_DTYPE)
        rec["status"] = abi.READ_NONE
        todo = np.nonzero(tk["status"] == abi.READ_ISSUED)[0]
        for attempt in range(2):
            if not len(todo):
                break
            rec[todo] = self.engine.serve_reads(g[todo], tk[todo], k[todo])
            todo = todo[rec["status"][todo] == abi.READ_BEHIND]
            if attempt == 0 and len(todo):
                # the BEHIND groups only: one apply per run of consecutive group ids
                ids_ = np.unique(g[todo])
                cuts = np.nonzero(np.diff(ids_) != 1)[0] + 1
                for run in np.split(ids_, cuts):
                    self.apply_committed(int(run[0]), len(run))
        if assert_leadership:
            ids_ = np.unique(g[tk["status"] == abi.READ_TERM_UNCOMMITTED])
            for run in np.split(ids_, np.nonzero(np.diff(ids_) != 1)[0] + 1) if len(ids_) else ():
                self.assert_leadership(int(run[0]), len(run))
        self.last_read = (tk, rec)
        name = self.commands.name
        return [(name(v), "SERVED") if s == abi.READ_SERVED else
                (None, abi.READ_TICKET_STATUS_NAMES[t] if s == abi.READ_NONE else abi.READ_STATUS_NAMES[s])
                for v, s, t in zip(rec["value"].tolist(), rec["status"].tolist(), tk["status"].tolist())]

    # -- crash and restart: the JVM of a node killed and relaunched (RaftServer.kt:302-310) ---
    def restart(self, groups, replicas, amnesia: bool = False, replay: bool = False, down_steps: int = 0) -> dict:
        """Restart node replicas[m] of groups[m], all in one device call (a
        node named twice restarts once): the mask of RaftEngine.restart over
        the span of the named groups.  Returns its info.  down_steps isolates
        the lowest restarted node of each group; isolate() cuts a node off
        without restarting it."""
        g = np.asarray(groups, dtype=np.int64).reshape(-1)
        r = np.asarray(replicas, dtype=np.int64).reshape(-1)
        if g.shape != r.shape:
            raise ValueError(f"restart: groups {g.shape} and replicas {r.shape} must be of one length")
        if g.size == 0:
            return {"restarted": 0, "leaders": 0, "entries_dropped": 0}
        if g.min() < 0 or g.max() >= self.engine.G or r.min() < 0 or r.max() >= self.engine.R:
            raise IndexError("restart: a node outside the engine")
        g0 = int(g.min())
        mask = np.zeros(int(g.max()) - g0 + 1, dtype=np.uint8)
        np.bitwise_or.at(mask, g - g0, (1 << r).astype(np.uint8))
        return self.engine.restart(mask, g0=g0, amnesia=amnesia, replay=replay, down_steps=down_steps)

    # -- scripted network faults: a node's cable pulled and put back (the reference has no counterpart) ---
    def isolate(self, groups, replicas, steps, replace: bool = False) -> np.ndarray:
        """Cut node replicas[m] of groups[m] off from its group for `steps`
        (RaftEngine.isolate: one device call, one isolated node per group, per
        group the first message counts).  replicas="leader" names each group's
        newest leader -- the one a linearizable read asks -- and
        "lowest_leader" the one RaftService.leader returns.  Returns the
        tickets; ``last_isolate`` keeps them."""
        sel = {"leader": abi.ISOLATE_NEWEST_LEADER, "lowest_leader": abi.ISOLATE_LOWEST_LEADER}
        if isinstance(replicas, str):
            if replicas not in sel:
                raise ValueError(f"isolate: replicas must be node indices, 'leader' or 'lowest_leader', not {replicas!r}")
            replicas = sel[replicas]
        else:
            replicas = np.asarray(replicas)
            if replicas.size and (replicas.min() < 0 or replicas.max() >= self.engine.R):
                raise IndexError("isolate: a node outside the engine")
        self.last_isolate = self.engine.isolate(np.asarray(groups, dtype=np.int64).reshape(-1), replicas, steps,
                                                replace=replace)
        return self.last_isolate

    def heal_network(self) -> dict:
        """Put every pulled cable back (RaftEngine.heal_network over every group):
        healed, idle, kept.  A healed stale leader steps down when it hears of
        the new term, a step or a heartbeat later."""
        return self.engine.heal_network()

    def isolated(self) -> List[tuple]:
        """The nodes cut off right now as (RaftNode, its state name, steps
        remaining), in group order (RaftEngine.isolated)."""
        _, rec = self.engine.isolated()
        names = ("FOLLOWER", "CANDIDATE", "LEADER")
        return [(RaftNode(self, int(g), int(r)), names[role] if 0 <= role < 3 else "?", int(rem))
                for g, r, role, rem in rec.tolist()]

    # -- persistence: what a node writes to disk before it answers (Raft paper fig. 2, "persistent state") ---
    def persist(self, max_records: Optional[int] = None) -> dict:
        """Bring this service's WalImage (``wal_image``, the stand-in for every
        node's disk) up to date: RaftWal.poll of every group until nothing is
        pending, each batch applied to the image.  Only what changed since the
        last call crosses the bus (etcd's Ready.HardState and Ready.Entries).
        The stream (``wal``) and the image are made at the first call.  Returns
        the polls' totals (delivered, hardstates, truncates, entries, lost,
        regressed); ``last_persist`` keeps them.  After RaftEngine.reset call
        ``wal.reset()`` and drop ``wal_image``."""
        e = self.engine
        if getattr(self, "wal", None) is None:
            self.wal = e.wal()
        if getattr(self, "wal_image", None) is None:
            self.wal_image = WalImage(e.G, e.R, e.cap, ring=int(e.p.log_window) > 0)
        tot = {k: 0 for k in ("delivered", "hardstates", "truncates", "entries", "lost", "regressed")}
        while True:
            rec, info = self.wal.poll(max_records=max_records)
            self.wal_image.apply(rec)
            for k in tot:
                tot[k] += info[k]
            if not info["pending"]:
                break
            if not info["delivered"]:
                raise ValueError("persist: max_records leaves no room for a record")
        self.last_persist = tot
        return tot

    def recover(self, group: int, replica: int) -> dict:
        """Give node `replica` of `group` back what it had persisted (the image
        as of the last persist()): currentTerm, votedFor and its log, with
        lastIndex and the physical length set to the image's length -- what a
        node with a disk reads at startup, e.g. after restart(amnesia=True) took
        it all.  Its volatile state (role, commitIndex, timers, sessions) stays
        as the restart left it.  One group's read_state / write_state /
        write_log; returns {"term", "vote", "length"}."""
        if getattr(self, "wal_image", None) is None:
            raise ValueError("recover: nothing was persisted (persist() first)")
        e, im = self.engine, self.wal_image
        if not (0 <= group < e.G and 0 <= replica < e.R):
            raise IndexError((group, replica))
        n = int(im.length[group, replica])
        st = e.read_state(group, 1)
        t, c = e.read_log(group, 1)
        t[0, replica], c[0, replica] = im.terms[group, replica], im.cmds[group, replica]
        t[0, replica, n:], c[0, replica, n:] = 0, 0
        base = replica * abi.NUM_FIELDS
        for name, v in (("term", im.term[group, replica]), ("voted", im.vote[group, replica]), ("last", n), ("phys", n)):
            st[0, base + abi.F_INDEX[name]] = int(v)
        e.write_log(t, c, group)
        e.write_state(st, group)
        return {"term": int(im.term[group, replica]), "vote": int(im.vote[group, replica]), "length": n}

    def recover_on_device(self, nodes) -> dict:
        """recover for many nodes at once, without a host copy of a group:
        `nodes` is a sequence of (group, replica) pairs (one named twice counts
        once); their replay.image_records, in (group, replica) order, are one
        replay.replay.  Each node gets back the image's currentTerm,
        votedFor and log and comes up as a restarted node does (FOLLOWER,
        commitIndex 0, a fresh election timeout); the other nodes do not
        change.  Of a ring image longer than the log_window only the newest
        log_window entries are sent, and no TRUNCATE: the node's lastIndex must
        then be at or below the first of them, as after restart(amnesia=True).
        Returns the replay's info."""
        if getattr(self, "wal_image", None) is None:
            raise ValueError("recover_on_device: nothing was persisted (persist() first)")
        e, im = self.engine, self.wal_image
        pairs = sorted({(int(g), int(r)) for g, r in nodes})
        if any(not (0 <= g < e.G and 0 <= r < e.R) for g, r in pairs):
            raise IndexError("recover_on_device: a node outside the engine")
        W = int(e.p.log_window)
        parts = []
        for g, r in pairs:
            rec = replay.image_records(im, g, r)
            if W and len(rec) - 2 > W:
                rec = np.concatenate([rec[:1], rec[-W:]])
            parts.append(rec)
        batch = np.concatenate(parts) if parts else np.zeros(0, dtype=abi.WAL_RECORD_DTYPE)
        return replay.replay(e, batch)

    def standby(self, other: "RaftService", max_records: Optional[int] = None) -> dict:
        """Bring `other`'s engine (same R, mode, log_cap and log_window, never
        stepped) up to this engine's persistent state: RaftWal.poll of this
        service's stream (``wal``, made at the first call) and replay.replay
        with keep_volatile into other.engine, until nothing is pending.  ``wal``
        is the stream persist() uses: a service feeds its image or a standby,
        not both.  Returns the totals (polls, applied, hardstates, truncates,
        entries, lost)."""
        if getattr(self, "wal", None) is None:
            self.wal = self.engine.wal()
        tot = {k: 0 for k in ("polls", "applied", "hardstates", "truncates", "entries", "lost")}
        while True:
            rec, info = self.wal.poll(max_records=max_records)
            done = replay.replay(other.engine, rec, keep_volatile=True)
            tot["polls"] += 1
            tot["lost"] += info["lost"]
            for k in ("applied", "hardstates", "truncates", "entries"):
                tot[k] += done[k]
            if not info["pending"]:
                return tot
            if not info["delivered"]:
                raise ValueError("standby: max_records leaves no room for a record")

    # -- leadership transfer (Raft thesis §3.10; the reference's leader only loses leadership by timeout) ---
    def transfer_leadership(self, group: int, to: Optional[int] = None) -> str:
        """Move `group`'s leadership to node `to` (None: the first caught-up idle
        follower after the leader, cyclically): its election timer fires in the
        next step.  Returns the ticket's status name ("SENT", "NO_LEADER", "SELF",
        "BEHIND", "BUSY", "UNREACHABLE", "NO_TARGET", "INVALID"); ``last_transfer``
        keeps the ticket for RaftEngine.resolve_transfers."""
        self.last_transfer = self.engine.transfer([group], [abi.TRANSFER_AUTO if to is None else to])
        return abi.TRANSFER_TICKET_STATUS_NAMES[int(self.last_transfer["status"][0])]

    def drain_node(self, replica: int, max_steps: int) -> int:
        """Vacate node `replica` in every group before a planned restart of it:
        while the leader directory (RaftEngine.leaders) names it in some group
        and the budget lasts, one evacuate of that replica over every group and
        one step.  Returns how many groups it still leads; ``last_drain`` keeps
        the turns taken and each turn's evacuate info.  A node that isolate()
        (or a restart's down_steps) has cut off is UNREACHABLE as a target and
        counts under an evacuate's busy."""
        e = self.engine
        if not 0 <= replica < e.R:
            raise IndexError(replica)
        mask = np.full(e.G, 1 << replica, dtype=np.uint8)
        infos = []
        remaining = int((e.leaders()["leader"] == replica).sum())
        while remaining and len(infos) < max_steps:
            infos.append(e.evacuate(mask))
            e.step(1)
            remaining = int((e.leaders()["leader"] == replica).sum())
        self.last_drain = {"turns": len(infos), "infos": infos}
        return remaining

    # -- snapshot install (Raft paper §7; the reference has none) -----------------------------
    def heal(self, min_lag: Optional[int] = None) -> dict:
        """Bring every replica that fell far behind back from its group's newest
        leader: one apply_committed, so that each leader's machine (the snapshot)
        holds its whole committed prefix, then one install_snapshot of every
        group.  min_lag: how many entries behind the leader's lastIndex a replica
        must be; by default half a log_window on a ring (the replica is about
        to lose the leader's window) and a quarter of log_cap on a flat log.
        Returns the install's info; ``last_heal_apply`` keeps the apply's."""
        e = self.engine
        if min_lag is None:
            W = int(e.p.log_window)
            min_lag = W // 2 if W else e.cap // 4
        self.last_heal_apply = self.apply_committed()
        return e.install_snapshot(min_lag=min_lag)

    # -- the client path: /cmd/{command} (RaftServer.kt:87-88) with an answer ---
    def leader(self, group: int) -> Optional[RaftNode]:
        """The group's leader node (the lowest id when there are several), or
        None: one 16-byte read, not RaftNode.state on every replica."""
        r = int(self.engine.leaders(group, 1)["leader"][0])
        return None if r < 0 else RaftNode(self, group, r)

    # -- the leader watch: a routing table kept from deltas (etcd's SoftState, TiKV's role observer) ---
    def watch_leaders(self, max_events: Optional[int] = None) -> np.ndarray:
        """Bring the cached leader directory up to date: one RaftEngine.poll_leaders
        of every group, its events (abi.EVENT_DTYPE, ascending group order)
        applied to ``leader_of`` / ``term_of`` -- two numpy arrays, one entry
        per group, (-1, 0) where the group has no leader -- and returned.  Only
        the groups whose newest leader or term changed since the last call
        cross the bus.  With max_events the rest stays pending for the next
        call; ``last_watch`` keeps the poll's info.  The directory mirrors the
        engine's watch: this service must be its only consumer, and after
        RaftEngine.reset or write_watch it starts over (``del leader_of``)."""
        if not hasattr(self, "leader_of"):
            self.leader_of = np.full(self.engine.G, -1, dtype=np.int32)
            self.term_of = np.zeros(self.engine.G, dtype=np.int32)
        self.last_watch, ev = self.engine.poll_leaders(max_events=max_events)
        self.leader_of[ev["group"]] = ev["leader"]
        self.term_of[ev["group"]] = ev["term"]
        return ev

    def newest_leader(self, group: int) -> Optional[RaftNode]:
        """The group's newest leader node as of the last watch_leaders (the
        LEADER of the highest term, never a deposed one that still holds the
        role), or None: a lookup in the cached directory, no device call."""
        if not 0 <= group < self.engine.G:
            raise IndexError(group)
        r = int(self.leader_of[group]) if hasattr(self, "leader_of") else -1
        return None if r < 0 else RaftNode(self, group, r)

    # -- the safety audit: did safety hold, and if not, in which groups and since when ------------------
    def check_safety(self, g0: int = 0, n: Optional[int] = None) -> dict:
        """Observe groups [g0, g0 + n) with this service's safety audit
        (RaftEngine.audit, made at the first call): the state now against what
        the audit remembers of earlier calls.  Returns the observe's info --
        newly_flagged, flagged, one count per kind (abi.AUDIT_KINDS), unknown;
        ``last_safety`` keeps it.  flagged == 0 in textbook mode without
        amnesia restarts; otherwise `violations` says where and since when.
        After RaftEngine.reset call ``safety_audit.reset()`` too."""
        if getattr(self, "safety_audit", None) is None:
            self.safety_audit = self.engine.audit()
        self.last_safety = self.safety_audit.observe(g0, n)
        return self.last_safety

    def violations(self, max_events: Optional[int] = None) -> np.ndarray:
        """The groups check_safety has flagged so far (abi.AUDIT_EVENT_DTYPE:
        group, flags of abi.AUDIT_*, first_step), in ascending group order, at
        most max_events of them.  Nothing is consumed; empty before the first
        check_safety."""
        if getattr(self, "safety_audit", None) is None:
            return np.zeros(0, dtype=abi.AUDIT_EVENT_DTYPE)
        return self.safety_audit.report(max_events=max_events)[1]

    # -- the liveness monitor: which groups make no progress now, for how long, and why -----------------
    def check_liveness(self, g0: int = 0, n: Optional[int] = None) -> dict:
        """Observe groups [g0, g0 + n) with this service's liveness monitor
        (``liveness_monitor``; RaftEngine.monitor() with its defaults, made at
        the first call unless the caller stored one with thresholds of its
        own).  Returns the observe's info -- flagged, newly_flagged, cleared,
        one count per kind (abi.MONITOR_KINDS), down, outages_ended,
        down_steps_ended; ``last_liveness`` keeps it with the range.  After
        RaftEngine.reset call ``liveness_monitor.reset()`` too."""
        if getattr(self, "liveness_monitor", None) is None:
            self.liveness_monitor = self.engine.monitor()
        info = self.liveness_monitor.observe(g0, n)
        self.last_liveness = (info, int(g0), self.engine.G - int(g0) if n is None else int(n))
        return info

    def unavailable(self, kinds: Optional[int] = None, max_events: Optional[int] = None) -> np.ndarray:
        """The groups the last check_liveness found stuck (abi.MONITOR_EVENT_DTYPE:
        group, now, ever, down_since, stall_since, leader, lag_mask) with a bit
        of `kinds` (an OR of abi.MONITOR_*; None: any) in `now`, in ascending
        group order, at most max_events of them.  Nothing is consumed; empty
        before the first check_liveness."""
        if getattr(self, "liveness_monitor", None) is None:
            return np.zeros(0, dtype=abi.MONITOR_EVENT_DTYPE)
        return self.liveness_monitor.report(max_events=max_events, kinds=kinds)[1]

    def remediate(self) -> dict:
        """Aim the engine's remedies at what the last check_liveness counted,
        over its range: if it counted commit_stalled groups and the engine runs
        in textbook mode, assert_leadership (a leader's no-op entry frees a
        commit an election left stuck); if it counted lagging groups and the
        machine is configured, heal's apply_committed and install_snapshot with
        min_lag = the monitor's lag_entries.  Returns {"noops": info or None,
        "install": info or None}.  The engine is never stepped: the remedies
        take effect in the caller's next steps."""
        out = {"noops": None, "install": None}
        if getattr(self, "last_liveness", None) is None:
            return out
        info, g0, n = self.last_liveness
        e = self.engine
        if info["commit_stalled"] and int(e.p.mode) == abi.MODE_TEXTBOOK:
            out["noops"] = self.assert_leadership(g0, n)
        if info["lagging"] and e.sm_slots:
            self.last_heal_apply = self.apply_committed(g0, n)
            out["install"] = e.install_snapshot(g0=g0, n=n, min_lag=self.liveness_monitor.config["lag_entries"])
        return out

    def submit(self, groups, commands: List[str]) -> np.ndarray:
        """One command per entry of `groups`, routed to each group's leader in
        the order given; returns the tickets (abi.TICKET_DTYPE).  A ticket with
        status abi.PROPOSE_NO_LEADER or PROPOSE_LOG_FULL stored nothing: the
        client retries it later."""
        return self.engine.propose(groups, [self.commands.intern(c) for c in commands])

    def status(self, groups, tickets, commands: List[str]) -> List[str]:
        """What became of each submitted command: "COMMITTED", "PENDING", "LOST",
        "NONE" (nothing was stored), "UNKNOWN" (log_window: the slot left a
        window).  ``last_status`` keeps the records (holders, committed_on, unknown)."""
        self.last_status = self.engine.resolve(groups, tickets, [self.commands.intern(c) for c in commands])
        return [abi.TICKET_STATUS_NAMES[s] for s in self.last_status["status"].tolist()]

    # -- reliable submission: the engine's proposal outbox (Raft thesis §6.3, "the client retries") ---
    def submit_reliable(self, groups, commands: List[str]) -> np.ndarray:
        """Queue one command per entry of `groups` in the engine's outbox
        (RaftEngine.outbox_configure first) and return their tags (int64, this
        service's own running numbers).  Nothing is proposed before the next
        completions() / pump_until_idle(): a pump proposes the new records and
        re-proposes the ones no replica holds any more, and never one that
        another replica might still commit, so a command commits once."""
        n0 = getattr(self, "_next_tag", 0)
        tags = np.arange(n0, n0 + len(commands), dtype=np.int64)
        ids = [self.commands.intern(c) for c in commands]
        self.engine.outbox_submit(groups, ids, tags)
        self._next_tag = n0 + len(commands)
        self._tag_cmd = getattr(self, "_tag_cmd", {})
        self._tag_cmd.update(zip(tags.tolist(), ids))
        return tags

    def completions(self, max_done: Optional[int] = None) -> List[tuple]:
        """One RaftEngine.outbox_pump: (tag, command, status, index, term, tries,
        age) per record that completed, in queue order; status is "COMMITTED"
        (at log[index] with `term`) or "EXPIRED" (outcome unknown, as after any
        client timeout).  ``last_pump`` keeps the pump's info."""
        self.last_pump, done = self.engine.outbox_pump(max_done)
        cmd = getattr(self, "_tag_cmd", {})
        return [(int(r["tag"]), self.commands.name(cmd.pop(int(r["tag"]))), abi.OUTBOX_DONE_NAMES[int(r["status"])],
                 int(r["index"]), int(r["term"]), int(r["tries"]), int(r["age"])) for r in done]

    def pump_until_idle(self, max_steps: int) -> List[tuple]:
        """Step and pump until the outbox is empty or max_steps steps were
        taken; a pump that left only PENDING records is followed by
        assert_leadership(), since an idle group commits entries of earlier
        terms only behind one of its leader's own.  Returns the completions."""
        out = self.completions()
        steps = 0
        while self.last_pump["left"] and steps < max_steps:
            if self.last_pump["left"] == self.last_pump["pending"]:
                self.assert_leadership()
            self.engine.step(1, counters=False)
            steps += 1
            out += self.completions()
        return out

    # -- the gRPC-facing wire form (include/raft_wire.h) --------------------
    # RaftImplBase.vote()/append() (RaftServer.kt:228, :253) receive and return
    # serialized protobufs; these batch them through the engine unchanged.
    def vote_wire(self, groups, replicas, requests: List[bytes]) -> List[bytes]:
        """Serialized RequestVoteRPCs -> serialized ResponseVoteRPCs."""
        q = wire.decode_vote_requests(requests)
        return wire.encode_vote_responses(self.engine.vote_batch(groups, replicas, q))

    def append_wire(self, groups, replicas, requests: List[bytes]) -> List[Optional[bytes]]:
        """Serialized RequestAppendEntriesRPCs -> serialized responses; None where
        the handler threw (Log.get, RaftServer.kt:276): that call has no response,
        which the reference's caller swallows (RaftServer.kt:170-172)."""
        rows, cmds, _ = wire.decode_append_requests(requests)
        rows = rows.astype(np.int64)
        for m, c in enumerate(cmds):
            if c is not None:
                rows[m, 6] = self.commands.intern(c.decode("utf-8"))
        out = self.engine.append_batch(groups, replicas, rows)
        enc = wire.encode_append_responses(out)
        return [None if out[m, 2] else enc[m] for m in range(len(enc))]
