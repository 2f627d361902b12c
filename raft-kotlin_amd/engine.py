"""RaftEngine — host-side handle of the HIP batched Raft engine (C-ABI in include/raft_engine.h).

One engine owns G groups x R replicas of Raft node state in the HBM of one
GPU.  ``step(n)`` advances every group by n lockstep heartbeat periods, which
is what each reference node does on its own timers
(RaftServer.kt:109-226, Commons.kt:10-31); the handler batches are the
reference's gRPC service (RaftServer.vote / RaftServer.append,
RaftServer.kt:228-287) applied to chosen replicas.

There is no CPU fallback anywhere in this module: every call goes to the HIP
library and a missing library or device raises.
"""
from __future__ import annotations

import ctypes as C
import weakref

import numpy as np

from . import abi


class RaftError(RuntimeError):
    pass


# -- what the wrappers share: argument checks, the DEVICE-pointer prologue, the record streams ---------------
def _int(what: str, name: str, v, lo=None, hi=None, allow_none: bool = False, want: str | None = None):
    """v as an int (None stays None with allow_none), or a ValueError that
    starts with the method's name.  A bool is never an integer; lo / hi bound
    the value (both inclusive); `want` words the message's demand."""
    if v is None and allow_none:
        return None
    if (isinstance(v, (int, np.integer)) and not isinstance(v, bool)
            and (lo is None or v >= lo) and (hi is None or v <= hi)):
        return int(v)
    if want is None:
        want = "an integer" + (f" in {lo}..{hi}" if hi is not None else f" >= {lo}" if lo is not None else "")
    raise ValueError(f"{what}: {name} must be {'None or ' if allow_none else ''}{want}, not {v!r}")


def _span(what: str, G: int, g0, n):
    """The group range [g0, g0 + n) of a call (n None: up to group G) as two
    ints.  Whether it lies inside the engine is the library's to refuse."""
    g0 = _int(what, "g0", g0)
    return g0, _int(what, "n", G - g0 if n is None else n)


def _dev_prologue(what: str, ptrs: dict, align: int = 16, after_stream=None, wait=None):
    """What a call on DEVICE pointers does first: the alignment of the named
    buffers, then `wait(after_stream)` (RaftEngine.wait_stream) when a stream
    was given."""
    if any(p % align for p in ptrs.values()):
        raise ValueError(f"{what}: the {' and '.join(ptrs)} buffer{'s' if len(ptrs) > 1 else ''} must be "
                         f"{align}-byte aligned")
    if after_stream is not None:
        wait(after_stream)


def _stream_call(owner, name: str, *args):
    """The closure a _RecordStream drives: one call of owner's entry point
    `name` (handle, *args, records, room, info), which returns its code.  The
    library is looked up when it is called, after every argument check."""
    return lambda out, room, info: getattr(owner._lib, name)(owner._h, *args, out, room, info)


class _RecordStream:
    """The protocol of every entry point that hands out ordered records cut at
    a room limit (include/raft_engine.h: drain_committed, poll_leaders,
    list_isolated, audit / monitor report, wal_poll), in one place.  `info` is
    the call's info struct (it has delivered and pending) and `fields` what
    of it the caller gets (None: its scalar fields), `dtype` the record,
    `align` what a DEVICE buffer of them needs, `noun` the name of the room
    argument.  A code in `survivable` is not raised: the call did everything
    else, and the info dict carries it as "status" (only such streams have
    the key).  `call` is a closure (records, room, info) -> code; `check`
    raises for a code (RaftEngine._check)."""

    def __init__(self, info, dtype, align: int, noun: str, fields=None, survivable=()):
        self.info, self.dtype, self.align, self.noun = info, dtype, align, noun
        self.fields, self.survivable = fields, tuple(survivable)

    def once(self, check, label: str, call, out_ptr, room) -> dict:
        """One call; a null out_ptr (with room 0) is a peek, which stores nothing."""
        info = self.info()
        rc = call(C.c_void_p(out_ptr or 0), int(room), C.byref(info))
        if rc not in self.survivable:
            check(rc, label)
        d = abi.info_dict(info, self.fields)
        if self.survivable:
            d["status"] = int(rc)
        return d

    def host(self, check, what: str, call, room, peek: bool = False, label: str | None = None):
        """(info, records) into a numpy array of at most `room` records (None:
        as many as there are -- a peek sizes the buffer); peek=True: the peek
        alone and no record."""
        _int(what, self.noun, room, lo=0, allow_none=True)
        label = label or what
        if peek:
            return self.once(check, label, call, 0, 0), np.zeros(0, dtype=self.dtype)
        if room is None:
            room = self.once(check, label, call, 0, 0)["pending"]
        # room 0 with a buffer is a call like any other (it stores what a delivery stores), not a peek: never a
        # null buffer
        out = np.zeros(max(1, int(room)), dtype=self.dtype)
        info = self.once(check, label, call, out.ctypes.data, room)
        return info, out[: info["delivered"]]

    def dev(self, check, what: str, call, out_ptr, room, after_stream=None, wait=None, label: str | None = None) -> dict:
        """The info of one call into a DEVICE buffer of `room` records."""
        _int(what, self.noun, room, lo=0, allow_none=True)
        if room is None or (room > 0 and not out_ptr):
            raise ValueError(f"{what}: a device buffer and its {self.noun} are required")
        _dev_prologue(what, {"record": out_ptr}, self.align, after_stream, wait)
        return self.once(check, label or what, call, out_ptr, room)


_DRAIN = _RecordStream(abi.raft_drain_info, abi.APPLIED_DTYPE, 8, "max_entries", survivable=(abi.RAFT_EWINDOW,))
_WATCH = _RecordStream(abi.raft_watch_info, abi.EVENT_DTYPE, 8, "max_events")
_ISOLATED = _RecordStream(abi.raft_isolated_info, abi.ISOLATED_DTYPE, 16, "max_events")
_AUDIT_REPORT = _RecordStream(abi.raft_audit_report_info, abi.AUDIT_EVENT_DTYPE, 16, "max_events")
_MONITOR_REPORT = _RecordStream(abi.raft_monitor_report_info, abi.MONITOR_EVENT_DTYPE, 16, "max_events")
_WAL = _RecordStream(abi.raft_wal_info, abi.WAL_RECORD_DTYPE, 8, "max_records", survivable=(abi.RAFT_EWINDOW,))


class RaftComm:
    """An RCCL communicator for the counter all-reduce of a sharded run
    (include/raft_engine.h raft_comm_*): rank 0 makes `unique_id()`, every
    rank gets it (any channel) and constructs RaftComm(uid, nranks, rank,
    device); construction returns once every rank has joined."""

    @staticmethod
    def unique_id() -> bytes:
        lib = abi.load_library()
        buf = (C.c_uint8 * abi.COMM_ID_BYTES)()
        if lib.raft_comm_get_unique_id(buf) != abi.RAFT_OK:
            raise RaftError("raft_comm_get_unique_id: " + lib.raft_last_error().decode(errors="replace"))
        return bytes(buf)

    def __init__(self, uid: bytes, nranks: int, rank: int, device: int = 0):
        self._lib = abi.load_library()
        if len(uid) != abi.COMM_ID_BYTES:
            raise ValueError(f"a communicator id is {abi.COMM_ID_BYTES} bytes")
        buf = (C.c_uint8 * abi.COMM_ID_BYTES).from_buffer_copy(uid)
        h = C.c_void_p()
        if self._lib.raft_comm_create(buf, nranks, rank, device, C.byref(h)) != abi.RAFT_OK:
            raise RaftError("raft_comm_create: " + self._lib.raft_last_error().decode(errors="replace"))
        self._h = h
        self.nranks, self.rank, self.device = nranks, rank, device

    def close(self):
        if getattr(self, "_h", None):
            self._lib.raft_comm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _GroupLedger:
    """What the handles that keep a ledger per group beside an engine share
    (RaftAudit, RaftMonitor, RaftWal): creating and closing the handle of the
    C functions named `_prefix`_*, device_bytes and reset, the group-range
    argument, the record stream, the ledgers as an int32 matrix, and closing
    on exit or collection."""

    _prefix = ""                                     # "raft_audit": the handle's functions are raft_audit_*

    def __init__(self, engine: "RaftEngine"):
        self._open(engine)

    def _fn(self, name: str):
        return getattr(self._lib, f"{self._prefix}_{name}")

    def _open(self, engine: "RaftEngine", *config):
        """`_prefix`_create(engine, *config, &handle)."""
        self._lib, self.engine = engine._lib, engine
        self.R, self.G = engine.R, engine.G
        h = C.c_void_p()
        engine._check(self._fn("create")(engine._h, *config, C.byref(h)), f"{self._prefix}_create")
        self._h = h

    def _check(self, rc: int, what: str):
        if rc != abi.RAFT_OK:
            raise RaftError(f"{what} failed ({rc}): " + self._lib.raft_last_error().decode(errors="replace"))

    def close(self):
        if getattr(self, "_h", None):
            self._fn("destroy")(self._h)                              # (RaftEngine.close closes its handles first)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @property
    def device_bytes(self) -> int:
        """HBM owned by the handle (RaftEngine.device_bytes does not count it)."""
        return int(self._fn("device_bytes")(self._h))

    def reset(self):
        """Back to the state as created: every ledger zero (a monitor's
        availability totals too), every cursor of a persistence stream fresh
        (its next poll sends everything)."""
        self._check(self._fn("reset")(self._h), f"{self._prefix[5:]} reset")

    def _range(self, g0, n, what: str):
        return _span(what, self.G, g0, n)

    def _observe(self, g0, n, info) -> dict:
        g0, n = self._range(g0, n, "observe")
        self._check(self._fn("observe")(self._h, g0, n, C.byref(info)), f"{self._prefix}_observe")
        return abi.info_dict(info)

    def _records(self, stream: _RecordStream, what: str, entry: str, args, room, dev: bool = False, out_ptr=None):
        """The handle's record stream `entry` (report, poll) with the call's
        leading arguments `args`: stream.host, or with dev=True stream.dev
        into out_ptr."""
        name = f"{self._prefix}_{entry}_dev" if dev else f"{self._prefix}_{entry}"
        call = _stream_call(self, name, *args)
        if dev:
            return stream.dev(self._check, what, call, out_ptr, room, label=name)
        return stream.host(self._check, what, call, room, label=name)

    def _read_words(self, g0, n) -> np.ndarray:
        n = self.G - g0 if n is None else n
        out = np.zeros((max(int(n), 0), self.words), dtype=np.int32)   # a bad range is the library's to refuse
        self._check(self._fn("read")(self._h, int(g0), int(n), abi.ptr(out, C.c_int32)), f"{self._prefix}_read")
        return out

    def _write_words(self, ledger, g0):
        a = np.asarray(ledger)
        if a.ndim != 2 or a.shape[1] != self.words or a.dtype.kind not in "iu":
            raise ValueError(f"{self._prefix[5:]} write: ledger {a.shape} {a.dtype} must be an integer array of shape "
                             f"(n, {self.words})")
        a = np.ascontiguousarray(a, dtype=np.int32)
        self._check(self._fn("write")(self._h, int(g0), a.shape[0], abi.ptr(a, C.c_int32)), f"{self._prefix}_write")


class RaftAudit(_GroupLedger):
    """A safety audit of one engine (include/raft_engine.h raft_audit_*): a
    ledger per group in HBM of its own, and `observe`, which checks the state
    now against it -- a term that went backwards, a vote changed within a
    term, two leaders of one term, a committed entry that changed, a newer
    leader that lacks it.  Made by RaftEngine.audit(); close it before its
    engine.  RaftEngine.reset does not reach it: call reset() here."""

    _prefix = "raft_audit"

    def __init__(self, engine: "RaftEngine"):
        self._open(engine)
        self.words = abi.audit_words(self.R)

    def observe(self, g0: int = 0, n: int | None = None) -> dict:
        """raft_audit_observe of groups [g0, g0 + n): check the state now
        against the ledger and advance the ledger.  Returns newly_flagged,
        flagged, one count per kind (abi.AUDIT_KINDS) of the groups that gained
        that bit in this call, and unknown (checks skipped below a log_window)."""
        return self._observe(g0, n, abi.raft_audit_info())

    def report(self, g0: int = 0, n: int | None = None, max_events: int | None = None):
        """raft_audit_report: (info, events) -- the groups of [g0, g0 + n) with
        flags != 0 as a numpy array of abi.AUDIT_EVENT_DTYPE (group, flags,
        first_step) in ascending group order, at most max_events of them (None:
        all of them; 0: a peek).  info: delivered, pending, flagged.  Nothing
        is consumed: the same call returns the same events."""
        return self._records(_AUDIT_REPORT, "report", "report", self._range(g0, n, "report"), max_events)

    def report_dev(self, out_ptr: int, max_events: int, g0: int = 0, n: int | None = None) -> dict:
        """report into a DEVICE buffer of max_events 16-byte records (16-byte
        aligned); returns the info once the kernels finished."""
        return self._records(_AUDIT_REPORT, "report_dev", "report", self._range(g0, n, "report_dev"), max_events, True,
                             out_ptr)

    def read(self, g0: int = 0, n: int | None = None) -> np.ndarray:
        """The ledgers of groups [g0, g0 + n): [n, 8 + 2 R] int32 (abi.AUDIT_WORDS,
        then (currentTerm, votedFor) per replica)."""
        return self._read_words(g0, n)

    def write(self, ledger: np.ndarray, g0: int = 0):
        """Store the ledgers of groups [g0, g0 + len(ledger)) (resuming an
        audit): an integer [n, 8 + 2 R] array.  The library refuses unknown flag
        bits, a lead_replica outside -1..R-1 and an anchor_count outside
        0..log_cap, and stores nothing then."""
        self._write_words(ledger, g0)


class RaftMonitor(_GroupLedger):
    """A liveness monitor of one engine (include/raft_engine.h raft_monitor_*):
    a 16-word ledger per group in HBM of its own, and `observe`, which brings it
    up to date from the state now -- since when the group has no leader, since
    when its leader's backlog has not advanced, which replicas lag, whether its
    terms churn -- and keeps a histogram of the lengths of the outages that
    ended.  Made by RaftEngine.monitor(); close it before its engine.
    RaftEngine.reset does not reach it: call reset() here."""

    _prefix = "raft_monitor"
    words = abi.MONITOR_WORDS

    def __init__(self, engine: "RaftEngine", **thresholds):
        cfg = abi.raft_monitor_config()
        for k, v in thresholds.items():
            if k not in abi.MONITOR_CONFIG_FIELDS:
                raise TypeError(f"monitor: unknown threshold {k!r}")
            setattr(cfg, k, _int("monitor", k, v, 0, 2 ** 31 - 1))
        self.config = abi.info_dict(cfg)
        self._open(engine, C.byref(cfg))

    def observe(self, g0: int = 0, n: int | None = None) -> dict:
        """raft_monitor_observe of groups [g0, g0 + n): bring their ledgers up
        to date from the state now.  Returns flagged, newly_flagged, cleared,
        one count per kind (abi.MONITOR_KINDS) of the groups that carry the bit
        now, down (groups without a leader, flagged or not yet), and the
        outages that ended in this call with the sum of their lengths."""
        return self._observe(g0, n, abi.raft_monitor_info())

    def _selection(self, g0, n, ever: bool, kinds, what: str):
        """(g0, n, which word, kinds): the leading arguments of a report."""
        kinds = _int(what, "kinds", abi.MONITOR_ALL if kinds is None else kinds, 0, abi.MONITOR_ALL,
                     want="None or an OR of abi.MONITOR_* bits")
        return (*self._range(g0, n, what), abi.MONITOR_EVER if ever else abi.MONITOR_NOW, kinds)

    def report(self, g0: int = 0, n: int | None = None, max_events: int | None = None, *, ever: bool = False,
               kinds: int | None = None):
        """raft_monitor_report: (info, events) -- the groups of [g0, g0 + n)
        whose `now` word (ever=True: whose sticky `ever` word) has a bit of
        `kinds` (None: any), as a numpy array of abi.MONITOR_EVENT_DTYPE (group,
        now, ever, down_since, stall_since, leader, lag_mask) in ascending group
        order, at most max_events of them (None: all of them; 0: a peek).  info:
        delivered, pending, flagged.  Nothing is consumed."""
        return self._records(_MONITOR_REPORT, "report", "report", self._selection(g0, n, ever, kinds, "report"),
                             max_events)

    def report_dev(self, out_ptr: int, max_events: int, g0: int = 0, n: int | None = None, *, ever: bool = False,
                   kinds: int | None = None) -> dict:
        """report into a DEVICE buffer of max_events 32-byte records (16-byte
        aligned); returns the info once the kernels finished."""
        return self._records(_MONITOR_REPORT, "report_dev", "report",
                             self._selection(g0, n, ever, kinds, "report_dev"), max_events, True, out_ptr)

    def availability(self) -> dict:
        """raft_monitor_get_availability: hist ([32] int64; hist[k] counts the
        ended outages of 2^k .. 2^(k+1) - 1 steps), outages, down_steps."""
        av = abi.raft_monitor_availability()
        self._check(self._lib.raft_monitor_get_availability(self._h, C.byref(av)), "raft_monitor_get_availability")
        return {"hist": np.array(av.hist[:], dtype=np.int64), **abi.info_dict(av)}

    def set_availability(self, hist, outages: int, down_steps: int):
        """raft_monitor_set_availability (resuming a monitor): the library
        refuses a negative total and stores nothing then."""
        h = np.asarray(hist)
        if h.shape != (abi.MONITOR_HIST,) or h.dtype.kind not in "iu":
            raise ValueError(f"set_availability: hist {h.shape} {h.dtype} must be {abi.MONITOR_HIST} integers")
        av = abi.raft_monitor_availability()
        av.hist[:] = [int(x) for x in h]
        av.outages, av.down_steps = int(outages), int(down_steps)
        self._check(self._lib.raft_monitor_set_availability(self._h, C.byref(av)), "raft_monitor_set_availability")

    def read(self, g0: int = 0, n: int | None = None) -> np.ndarray:
        """The ledgers of groups [g0, g0 + n): [n, 16] int32 (abi.MONITOR_WORD_NAMES)."""
        return self._read_words(g0, n)

    def write(self, ledger: np.ndarray, g0: int = 0):
        """Store the ledgers of groups [g0, g0 + len(ledger)) (resuming a
        monitor): an integer [n, 16] array.  The library refuses unknown bits in
        now or ever, a leader outside -1..R-1, lag_mask bits at or above R, a
        negative count and nonzero reserved words, and stores nothing then."""
        self._write_words(ledger, g0)


class RaftWal(_GroupLedger):
    """The persistence stream of one engine (include/raft_engine.h raft_wal_*):
    a cursor per replica in HBM of its own, and `poll`, which hands out what a
    replica must make durable -- its hard state when it changed, a TRUNCATE
    when what was handed out is no longer its log, and the entries it gained
    since -- as records in (group, replica) order.  Apply them to a WalImage.
    Made by RaftEngine.wal(); close it before its engine.  RaftEngine.reset
    does not reach it: call reset() here."""

    _prefix = "raft_wal"

    def _selection(self, g0, n, replica, what: str):
        """(g0, n, replica): the leading arguments of a poll."""
        return (*self._range(g0, n, what),
                _int(what, "replica", replica, -1, self.R - 1, want=f"-1 (all) or in 0..{self.R - 1}"))

    def peek(self, g0: int = 0, n: int | None = None, replica: int = -1) -> dict:
        """What a poll would see, storing nothing: info with delivered = 0 and
        pending = every record of the selection."""
        call = _stream_call(self, "raft_wal_poll", *self._selection(g0, n, replica, "peek"))
        return _WAL.once(self._check, "raft_wal_poll", call, 0, 0)

    def poll(self, g0: int = 0, n: int | None = None, replica: int = -1, max_records: int | None = None):
        """raft_wal_poll of groups [g0, g0 + n) (replica -1: every replica, else
        that replica index): (records, info).  records is a numpy array of
        abi.WAL_RECORD_DTYPE (group, replica, kind, index, term, cmd, aux) in
        ascending (group, replica) order, HARDSTATE, TRUNCATE, then ENTRY
        ascending inside a replica; at most max_records of them (None: as many
        as there are -- a peek sizes the buffer).  The cursors advance past
        what was returned.  info: delivered, pending, hardstates, truncates,
        entries, lost, regressed, status: RAFT_EWINDOW is not raised, the call
        did everything else (info["lost"] > 0 says how many entries left the
        log window unread)."""
        info, records = self._records(_WAL, "poll", "poll", self._selection(g0, n, replica, "poll"), max_records)
        return records, info

    def poll_dev(self, out_ptr: int, max_records: int, g0: int = 0, n: int | None = None, replica: int = -1) -> dict:
        """poll into a DEVICE buffer of max_records 24-byte records (8-byte
        aligned); returns the info once the kernels finished."""
        return self._records(_WAL, "poll_dev", "poll", self._selection(g0, n, replica, "poll_dev"), max_records, True,
                             out_ptr)

    def cursors(self, g0: int = 0, n: int | None = None) -> np.ndarray:
        """The cursors of groups [g0, g0 + n): [n, R] of abi.WAL_CURSOR_DTYPE
        (term, vote, stable, stable_term, floor, pad)."""
        n = self.G - g0 if n is None else n
        out = np.zeros((max(int(n), 0), self.R), dtype=abi.WAL_CURSOR_DTYPE)   # a bad range is the library's to refuse
        self._check(self._lib.raft_wal_read(self._h, int(g0), int(n), C.c_void_p(out.ctypes.data)), "raft_wal_read")
        return out

    def set_cursors(self, cursors: np.ndarray, g0: int = 0):
        """Store the cursors of groups [g0, g0 + len(cursors)) (resuming a
        consumer): an [n, R] array of abi.WAL_CURSOR_DTYPE.  The library refuses
        a stable outside 0..log_cap, a floor outside 0..stable, a vote outside
        -1..R (a node id: replica index + 1), a negative term and a nonzero pad,
        and stores nothing then."""
        a = np.asarray(cursors)
        if a.ndim != 2 or a.shape[1] != self.R or a.dtype != abi.WAL_CURSOR_DTYPE:
            raise ValueError(f"set_cursors: cursors {a.shape} {a.dtype} must be abi.WAL_CURSOR_DTYPE of shape (n, {self.R})")
        a = np.ascontiguousarray(a)
        self._check(self._lib.raft_wal_write(self._h, int(g0), a.shape[0], C.c_void_p(a.ctypes.data)), "raft_wal_write")


class WalImage:
    """What a host keeps on disk: the image the records of RaftWal.poll build,
    in numpy only -- term [G, R], vote [G, R], length [G, R] and the entries
    terms / cmds [G, R, cap].  apply() refuses an ENTRY that is not at
    `length` and a TRUNCATE above `length`: a stream with a record missing or
    out of order fails loudly instead of building a wrong image.  With
    ring=True (an engine with a log_window) an ENTRY above `length` is
    accepted: the entries between left the window unpersisted (the poll
    counted them in `lost`) and stay zero in the image."""

    def __init__(self, G: int, R: int, cap: int, ring: bool = False):
        self.G, self.R, self.cap, self.ring = int(G), int(R), int(cap), bool(ring)
        self.term = np.zeros((G, R), np.int32)
        self.vote = np.full((G, R), -1, np.int32)
        self.length = np.zeros((G, R), np.int32)
        self.terms = np.zeros((G, R, cap), np.int32)
        self.cmds = np.zeros((G, R, cap), np.uint32)

    def apply(self, records: np.ndarray) -> int:
        """Apply records (abi.WAL_RECORD_DTYPE) in order; returns how many.
        Raises ValueError at the first record that does not fit the image,
        with the records before it applied."""
        rec = np.asarray(records)
        for m, (g, r, kind, index, term, cmd, aux) in enumerate(rec.tolist()):
            if not (0 <= g < self.G and 0 <= r < self.R):
                raise ValueError(f"record {m}: replica ({g}, {r}) outside the image")
            n = int(self.length[g, r])
            if kind == abi.WAL_HARDSTATE:
                self.term[g, r], self.vote[g, r] = term, aux
            elif kind == abi.WAL_TRUNCATE:
                if not 0 <= index <= n:
                    raise ValueError(f"record {m}: TRUNCATE({index}) of ({g}, {r}) above its length {n}")
                self.length[g, r] = index
            elif kind == abi.WAL_ENTRY:
                if not (index == n or (self.ring and n < index)) or index >= self.cap:
                    raise ValueError(f"record {m}: ENTRY {index} of ({g}, {r}) is not at its length {n}")
                self.terms[g, r, n:index], self.cmds[g, r, n:index] = 0, 0
                self.terms[g, r, index], self.cmds[g, r, index] = term, cmd
                self.length[g, r] = index + 1
            else:
                raise ValueError(f"record {m}: unknown kind {kind}")
        return len(rec)

    def log(self, g: int, r: int):
        """(terms, cmds) of replica r of group g: its persisted entries [0, length)."""
        n = int(self.length[g, r])
        return self.terms[g, r, :n].copy(), self.cmds[g, r, :n].copy()


class RaftEngine:
    def __init__(self, params: abi.raft_params, device: int = 0):
        self._lib = abi.load_library()
        self.p = params
        self.R = int(params.R)
        self.G = int(params.G)
        self.g0 = int(params.g0)
        self.cap = int(params.log_cap)
        self.W = abi.group_words(self.R)
        self.device = device
        h = C.c_void_p()
        self._check(self._lib.raft_engine_create(C.byref(params), device, C.byref(h)), "raft_engine_create")
        self._h = h

    # -- plumbing ---------------------------------------------------------
    def _check(self, rc: int, what: str):
        if rc != abi.RAFT_OK:
            msg = self._lib.raft_last_error().decode(errors="replace")
            raise RaftError(f"{what} failed ({rc}): {msg}")

    def _adopt(self, child):
        """Remember a handle made from this engine (an audit, a monitor, a
        persistence stream), weakly: close() closes it first."""
        self.__dict__.setdefault("_children", []).append(weakref.ref(child))
        return child

    def close(self):
        if getattr(self, "_h", None):
            for ref in getattr(self, "_children", ()):                # they go before their engine
                child = ref()
                if child is not None:
                    child.close()
            self._lib.raft_engine_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _dev(self, what: str, after_stream, align: int = 16, **ptrs):
        """The prologue of a call on DEVICE pointers: the alignment of the
        named buffers, then `after_stream`."""
        _dev_prologue(what, ptrs, align, after_stream, self.wait_stream)

    def _records_dev(self, stream: _RecordStream, what: str, name: str, args, out_ptr, room, after_stream) -> dict:
        return stream.dev(self._check, what, _stream_call(self, name, *args), out_ptr, room, after_stream, self.wait_stream)

    @staticmethod
    def _byte_mask(mask, n, what: str):
        """A mask of one byte per group as (contiguous uint8 array, n): the C
        side reads n bytes."""
        m = np.asarray(mask)
        if m.ndim != 1 or m.dtype.kind not in "iu" or (m.size and (m.min() < 0 or m.max() > 0xFF)):
            raise ValueError(f"{what}: mask {m.shape} {m.dtype} must be a 1-D array of byte values")
        n = m.shape[0] if n is None else n
        if m.shape[0] != n:
            raise ValueError(f"{what}: mask holds {m.shape[0]} groups, n is {n}")
        return np.ascontiguousarray(m, dtype=np.uint8), n

    @property
    def stream(self) -> int:
        """hipStream_t of the engine (for torch.cuda.ExternalStream / events)."""
        return int(self._lib.raft_engine_stream(self._h) or 0)

    @property
    def step_index(self) -> int:
        return int(self._lib.raft_engine_step_index(self._h))

    @step_index.setter
    def step_index(self, t: int):
        self._check(self._lib.raft_engine_set_step_index(self._h, int(t)), "set_step_index")

    def set_steps_per_launch(self, k: int):
        """Steps fused into one kernel launch from now on (results do not depend on it)."""
        self._check(self._lib.raft_engine_set_steps_per_launch(self._h, int(k)), "set_steps_per_launch")

    @property
    def subranges(self) -> int:
        """Launch sub-ranges in use (raft_params.subranges; streams per launch).
        An older experimental build (RAFT_ENGINE_LIB) without them: 1."""
        if getattr(self._lib.raft_engine_subranges, "__name__", "") == "stub":
            return 1
        return int(self._lib.raft_engine_subranges(self._h))

    def set_subranges(self, n: int):
        """Split the step launches over n sub-range streams (0 = automatic)."""
        if getattr(self._lib.raft_engine_set_subranges, "__name__", "") == "stub":
            return                                   # an older experimental build: one range
        self._check(self._lib.raft_engine_set_subranges(self._h, int(n)), "set_subranges")

    def set_kernel(self, kernel: int):
        """The step kernel variant from now on (abi.KERNEL_AUTO / KERNEL_GENERAL;
        results do not depend on it)."""
        self._check(self._lib.raft_engine_set_kernel(self._h, int(kernel)), "set_kernel")

    def set_batch_path(self, path: int):
        """How the handler batches order their messages (abi.BATCH_PATH_AUTO /
        _SORTED / _BUCKETED; results do not depend on it)."""
        self._check(self._lib.raft_engine_set_batch_path(self._h, int(path)), "set_batch_path")
        self._batch_path = int(path)

    @property
    def batch_path(self) -> int:
        """The batch path set with set_batch_path (abi.BATCH_PATH_AUTO unless set)."""
        return getattr(self, "_batch_path", abi.BATCH_PATH_AUTO)

    def reset(self):
        """Every group back to its initial state at step 0 (as created)."""
        self._check(self._lib.raft_engine_reset(self._h), "reset")

    def kernel_info(self) -> dict:
        """The step kernel and schedule of the last step launch
        (raft_engine_kernel_info): net (raft_step.h NET_* bits), textbook, ring,
        steps, workgroups, resident_workgroups, balanced (sub-ranges on the
        balanced schedule), subranges."""
        k = abi.raft_kernel_info()
        self._check(self._lib.raft_engine_kernel_info(self._h, C.byref(k)), "kernel_info")
        return abi.info_dict(k)

    @property
    def device_bytes(self) -> int:
        """HBM owned by the engine, the batch / accessor staging included."""
        return int(self._lib.raft_engine_device_bytes(self._h))

    def trim_staging(self):
        """Free the grow-only staging of the handler batches and accessors."""
        self._check(self._lib.raft_engine_trim_staging(self._h), "trim_staging")

    # -- the hot path -----------------------------------------------------
    def step(self, n: int = 1, counters: bool = True) -> np.ndarray | None:
        """Advance n lockstep steps; returns [n, NUM_COUNTERS] int64 counters."""
        c = abi.counters_array(n) if counters else None
        self._check(self._lib.raft_engine_step(self._h, n, abi.ptr(c, C.c_int64) if c is not None else None),
                    "raft_engine_step")
        return c[:, : abi.NUM_COUNTERS] if c is not None else None

    def step_async(self, n: int, counters_dev_ptr: int | None = None):
        """Enqueue n steps on the engine stream; counters to a device buffer
        of [n][COUNTER_STRIDE] int64 (e.g. a torch tensor's data_ptr())."""
        self._check(self._lib.raft_engine_step_async(self._h, n, C.c_void_p(counters_dev_ptr or 0)),
                    "raft_engine_step_async")

    def set_kernel_timing(self, enable: bool = True):
        """Bracket every step-kernel launch with HIP events on the engine stream."""
        self._check(self._lib.raft_engine_set_kernel_timing(self._h, int(enable)), "set_kernel_timing")

    def kernel_time(self):
        """(summed step-kernel ms, launches) since the last call; synchronises."""
        ms, n = C.c_double(), C.c_int64()
        self._check(self._lib.raft_engine_kernel_time(self._h, C.byref(ms), C.byref(n)), "kernel_time")
        return float(ms.value), int(n.value)

    def sync(self):
        self._check(self._lib.raft_engine_sync(self._h), "raft_engine_sync")

    # -- state ------------------------------------------------------------
    def read_state(self, g0: int = 0, n: int | None = None) -> np.ndarray:
        n = self.G - g0 if n is None else n
        out = np.zeros((n, self.W), dtype=np.int32)
        self._check(self._lib.raft_engine_read_state(self._h, g0, n, abi.ptr(out, C.c_int32)), "read_state")
        return out

    def write_state(self, state: np.ndarray, g0: int = 0):
        s = np.ascontiguousarray(state, dtype=np.int32).reshape(-1, self.W)
        self._check(self._lib.raft_engine_write_state(self._h, g0, s.shape[0], abi.ptr(s, C.c_int32)),
                    "write_state")

    def read_log(self, g0: int = 0, n: int | None = None):
        n = self.G - g0 if n is None else n
        t = np.zeros((n, self.R, self.cap), dtype=np.int32)
        c = np.zeros((n, self.R, self.cap), dtype=np.uint32)
        self._check(self._lib.raft_engine_read_log(self._h, g0, n, abi.ptr(t, C.c_int32), abi.ptr(c, C.c_uint32)),
                    "read_log")
        return t, c

    def write_log(self, terms: np.ndarray, cmds: np.ndarray, g0: int = 0):
        t = np.ascontiguousarray(terms, dtype=np.int32)
        c = np.ascontiguousarray(cmds, dtype=np.uint32)
        # the C side reads n * R * log_cap words from both arrays
        if t.ndim != 3 or t.shape[1:] != (self.R, self.cap) or c.shape != t.shape:
            raise ValueError(f"write_log: terms {t.shape} and cmds {c.shape} must both be (n, {self.R}, {self.cap})")
        self._check(self._lib.raft_engine_write_log(self._h, g0, t.shape[0], abi.ptr(t, C.c_int32),
                                                    abi.ptr(c, C.c_uint32)), "write_log")

    def digest(self) -> int:
        out = C.c_uint64()
        self._check(self._lib.raft_engine_digest(self._h, C.byref(out)), "digest")
        return int(out.value)

    def digest_range(self, g0: int, n: int) -> int:
        """The digest of groups [g0, g0 + n) only."""
        out = C.c_uint64()
        self._check(self._lib.raft_engine_digest_range(self._h, g0, n, C.byref(out)), "digest_range")
        return int(out.value)

    def check_log_matching(self, g0: int = 0, n: int | None = None, flags: bool = False):
        """Groups whose replicas disagree inside their common committed prefix
        (safety flag, include/raft_engine.h); returns the count, or (count,
        per-group uint8 flags) with flags=True."""
        n = self.G - g0 if n is None else n
        f = np.zeros(n, dtype=np.uint8) if flags else None
        out = C.c_int64()
        self._check(self._lib.raft_engine_check_log_matching(self._h, g0, n, abi.ptr(f, C.c_uint8) if flags else None,
                                                             C.byref(out)), "check_log_matching")
        return (int(out.value), f) if flags else int(out.value)

    # -- committed-entry delivery (lastApplied, RaftServer.kt:47) ------------
    def _replica_span(self, g0, n, replica, what: str):
        """(g0, n, replica) of a call on one replica index or all (-1), checked
        before any library call."""
        g0, n = _span(what, self.G, g0, n)
        return g0, n, _int(what, "replica", replica, -1, self.R - 1, want=f"-1 (all) or in 0..{self.R - 1}")

    def peek_committed(self, g0: int = 0, n: int | None = None, replica: int = -1) -> dict:
        """What a drain would see, storing nothing: info with delivered = 0 and
        pending = every committed, undelivered entry of the selection."""
        call = _stream_call(self, "raft_engine_drain_committed", *self._replica_span(g0, n, replica, "peek_committed"))
        return _DRAIN.once(self._check, "peek_committed", call, 0, 0)

    def drain_committed(self, g0: int = 0, n: int | None = None, replica: int = -1,
                        max_entries: int | None = None):
        """The entries of groups [g0, g0 + n) (replica -1: every replica, else
        that replica index) that became committed since they were last drained:
        (records, info).  records is a numpy array of abi.APPLIED_DTYPE (group,
        replica, index, term, cmd) in ascending (group, replica, index) order,
        at most max_entries of them (None: as many as there are -- a peek sizes
        the buffer); lastApplied advances past what was returned.  info:
        delivered, pending, lost, regressed, status (include/raft_engine.h):
        RAFT_EWINDOW is not raised, the call did everything else and the
        records are returned (info["lost"] > 0 says how many entries left the
        log window unread)."""
        call = _stream_call(self, "raft_engine_drain_committed", *self._replica_span(g0, n, replica, "drain_committed"))
        info, records = _DRAIN.host(self._check, "drain_committed", call, max_entries)
        return records, info

    def drain_committed_dev(self, out_ptr: int, max_entries: int, g0: int = 0, n: int | None = None,
                            replica: int = -1, after_stream: int | None = None) -> dict:
        """drain_committed into a DEVICE buffer of max_entries 24-byte records
        (e.g. a torch uint8 tensor's data_ptr() on this engine's GPU; 8-byte
        aligned); returns info once the kernels finished."""
        return self._records_dev(_DRAIN, "drain_committed_dev", "raft_engine_drain_committed_dev",
                                 self._replica_span(g0, n, replica, "drain_committed_dev"), out_ptr, max_entries,
                                 after_stream)

    def applied(self, g0: int = 0, n: int | None = None) -> np.ndarray:
        """lastApplied of groups [g0, g0 + n): [n, R] int32."""
        n = self.G - g0 if n is None else n
        out = np.zeros((max(int(n), 0), self.R), dtype=np.int32)     # a bad range is the library's to refuse
        self._check(self._lib.raft_engine_read_applied(self._h, int(g0), int(n), abi.ptr(out, C.c_int32)), "read_applied")
        return out

    def set_applied(self, applied: np.ndarray, g0: int = 0):
        """Store lastApplied of groups [g0, g0 + len(applied)) (resuming a
        consumer): an integer [n, R] array with every value in 0..log_cap."""
        a = np.asarray(applied)
        if a.ndim != 2 or a.shape[1] != self.R or a.dtype.kind not in "iu":
            raise ValueError(f"set_applied: applied {a.shape} {a.dtype} must be an integer array of shape (n, {self.R})")
        if a.size and (a.min() < 0 or a.max() > self.cap):
            raise ValueError(f"set_applied: every value must be in 0..{self.cap}")
        a = np.ascontiguousarray(a, dtype=np.int32)
        self._check(self._lib.raft_engine_write_applied(self._h, g0, a.shape[0], abi.ptr(a, C.c_int32)), "write_applied")

    # -- the client path: leader directory, routed proposals, tickets ---------
    def leaders(self, g0: int = 0, n: int | None = None) -> np.ndarray:
        """The leader directory of groups [g0, g0 + n): abi.LEADER_DTYPE records
        (leader: the lowest replica index with role LEADER or -1, its term and
        commitIndex, n_leaders) -- 16 bytes per group, no whole-state copy."""
        n = self.G - g0 if n is None else n
        out = np.zeros(max(int(n), 0), dtype=abi.LEADER_DTYPE)       # a bad range is the library's to refuse
        self._check(self._lib.raft_engine_read_leaders(self._h, int(g0), int(n), C.c_void_p(out.ctypes.data)),
                    "read_leaders")
        return out

    @staticmethod
    def _client_arrays(groups, cmds, what: str):
        """groups / cmds as contiguous int64 / uint32 vectors of one length
        (the C side reads n of each)."""
        g = np.ascontiguousarray(groups, dtype=np.int64)
        c = np.ascontiguousarray(cmds, dtype=np.uint32)
        if g.ndim != 1 or c.ndim != 1 or g.shape[0] != c.shape[0]:
            raise ValueError(f"{what}: groups {g.shape} and cmds {c.shape} must be 1-D and of one length")
        return g, c

    def _client_status(self, rc: int, what: str, allowed=(abi.RAFT_EWINDOW,)) -> int:
        """Raise on an error the call did not survive; a code in `allowed` (the
        call did everything else) is kept in ``last_status`` instead."""
        if rc not in allowed:
            self._check(rc, what)
        self.last_status = int(rc)
        return int(rc)

    def propose(self, groups, cmds) -> np.ndarray:
        """raft_propose_batch: command cmds[m] (a u32 id) to the leader of
        groups[m], in batch order; returns abi.TICKET_DTYPE tickets (replica,
        index, term, status = abi.PROPOSE_*).  RAFT_EWINDOW (a textbook add
        below a log_window) is not raised: the batch was applied, the tickets
        are returned and ``last_status`` carries the code."""
        g, c = self._client_arrays(groups, cmds, "propose")
        t = np.zeros(g.shape[0], dtype=abi.TICKET_DTYPE)
        self._client_status(self._lib.raft_propose_batch(self._h, C.c_void_p(g.ctypes.data), C.c_void_p(c.ctypes.data),
                                                         C.c_void_p(t.ctypes.data), g.shape[0]), "raft_propose_batch")
        return t

    def propose_dev(self, group_ptr: int, cmd_ptr: int, ticket_ptr: int, n: int,
                    after_stream: int | None = None) -> int:
        """raft_propose_batch_dev: DEVICE pointers to n int64 groups, uint32
        commands and 16-byte tickets (16-byte aligned); returns RAFT_OK or
        RAFT_EWINDOW once the batch finished."""
        self._dev("propose_dev", after_stream, ticket=ticket_ptr)
        return self._client_status(self._lib.raft_propose_batch_dev(self._h, group_ptr, cmd_ptr, ticket_ptr, int(n)),
                                   "raft_propose_batch_dev")

    def resolve(self, groups, tickets, cmds, check: bool = True) -> np.ndarray:
        """raft_engine_resolve_tickets: what became of each ticket's entry, as
        abi.TICKET_STATE_DTYPE records (status = abi.TICKET_*, holders,
        committed_on, unknown).  Read-only.  RAFT_EWINDOW (some record is
        UNKNOWN) is never raised; with check=False neither are RAFT_ERANGE /
        RAFT_EINVAL (some record is INVALID): ``last_status`` carries the code."""
        g, c = self._client_arrays(groups, cmds, "resolve")
        t = np.ascontiguousarray(tickets)
        if t.dtype != abi.TICKET_DTYPE or t.ndim != 1 or t.shape[0] != g.shape[0]:
            raise ValueError(f"resolve: tickets must be {g.shape[0]} records of abi.TICKET_DTYPE")
        out = np.zeros(g.shape[0], dtype=abi.TICKET_STATE_DTYPE)
        allowed = (abi.RAFT_EWINDOW,) if check else (abi.RAFT_EWINDOW, abi.RAFT_ERANGE, abi.RAFT_EINVAL)
        self._client_status(self._lib.raft_engine_resolve_tickets(
            self._h, C.c_void_p(g.ctypes.data), C.c_void_p(t.ctypes.data), C.c_void_p(c.ctypes.data),
            C.c_void_p(out.ctypes.data), g.shape[0]), "raft_engine_resolve_tickets", allowed)
        return out

    def resolve_dev(self, group_ptr: int, ticket_ptr: int, cmd_ptr: int, out_ptr: int, n: int,
                    after_stream: int | None = None) -> int:
        """raft_engine_resolve_tickets_dev on DEVICE pointers (tickets and
        records 16-byte aligned); returns RAFT_OK or RAFT_EWINDOW."""
        self._dev("resolve_dev", after_stream, ticket=ticket_ptr, record=out_ptr)
        return self._client_status(self._lib.raft_engine_resolve_tickets_dev(self._h, group_ptr, ticket_ptr, cmd_ptr,
                                                                             out_ptr, int(n)),
                                   "raft_engine_resolve_tickets_dev")

    # -- linearizable reads (raft_read_begin_batch*, raft_read_serve_batch*) --------
    def begin_reads(self, groups) -> np.ndarray:
        """raft_read_begin_batch: a read ticket per entry of `groups`, as
        abi.READ_TICKET_DTYPE records (replica: the group's newest leader, term,
        read_index: its committed prefix, status = abi.READ_ISSUED /
        READ_TERM_UNCOMMITTED / READ_NO_LEADER / READ_UNKNOWN).  Read-only.
        RAFT_EWINDOW (some ticket is UNKNOWN) is not raised: ``last_status``
        carries the code."""
        g = np.ascontiguousarray(groups, dtype=np.int64)
        if g.ndim != 1:
            raise ValueError(f"begin_reads: groups {g.shape} must be 1-D")
        t = np.zeros(g.shape[0], dtype=abi.READ_TICKET_DTYPE)
        self._client_status(self._lib.raft_read_begin_batch(self._h, C.c_void_p(g.ctypes.data), C.c_void_p(t.ctypes.data),
                                                            g.shape[0]), "raft_read_begin_batch")
        return t

    def begin_reads_dev(self, group_ptr: int, ticket_ptr: int, n: int, after_stream: int | None = None) -> int:
        """raft_read_begin_batch_dev: DEVICE pointers to n int64 groups and
        16-byte tickets (16-byte aligned); returns RAFT_OK or RAFT_EWINDOW."""
        self._dev("begin_reads_dev", after_stream, ticket=ticket_ptr)
        return self._client_status(self._lib.raft_read_begin_batch_dev(self._h, group_ptr, ticket_ptr, int(n)),
                                   "raft_read_begin_batch_dev")

    def serve_reads(self, groups, tickets, keys, check: bool = True) -> np.ndarray:
        """raft_read_serve_batch: register keys[m] (its low bits name the
        slot) of the replica tickets[m] names in groups[m], confirmed against
        the group's terms, as abi.READ_RESULT_DTYPE records (value, status =
        abi.READ_SERVED ... READ_INVALID, applied, agree).  Read-only; needs
        sm_configure.  With check=False RAFT_ERANGE / RAFT_EINVAL (some record
        is INVALID) are not raised: ``last_status`` carries the code."""
        g, k = self._client_arrays(groups, keys, "serve_reads")
        t = np.ascontiguousarray(tickets)
        if t.dtype != abi.READ_TICKET_DTYPE or t.ndim != 1 or t.shape[0] != g.shape[0]:
            raise ValueError(f"serve_reads: tickets must be {g.shape[0]} records of abi.READ_TICKET_DTYPE")
        out = np.zeros(g.shape[0], dtype=abi.READ_RESULT_DTYPE)
        # an unconfigured machine is RAFT_EINVAL too, and fills nothing: that one always raises
        allowed = () if check or not self.sm_slots else (abi.RAFT_ERANGE, abi.RAFT_EINVAL)
        self._client_status(self._lib.raft_read_serve_batch(
            self._h, C.c_void_p(g.ctypes.data), C.c_void_p(t.ctypes.data), C.c_void_p(k.ctypes.data),
            C.c_void_p(out.ctypes.data), g.shape[0]), "raft_read_serve_batch", allowed)
        return out

    def serve_reads_dev(self, group_ptr: int, ticket_ptr: int, key_ptr: int, out_ptr: int, n: int,
                        after_stream: int | None = None, check: bool = True) -> int:
        """raft_read_serve_batch_dev on DEVICE pointers (tickets and records
        16-byte aligned); returns the call's code (see serve_reads)."""
        self._dev("serve_reads_dev", after_stream, ticket=ticket_ptr, record=out_ptr)
        allowed = () if check or not self.sm_slots else (abi.RAFT_ERANGE, abi.RAFT_EINVAL)
        return self._client_status(self._lib.raft_read_serve_batch_dev(self._h, group_ptr, ticket_ptr, key_ptr, out_ptr,
                                                                       int(n)), "raft_read_serve_batch_dev", allowed)

    # -- the replicated state machine (raft_engine_sm_*) -------------------------
    @property
    def sm_slots(self) -> int:
        """Registers per replica of the configured state machine (0: none)."""
        return getattr(self, "_sm_slots", 0)

    def sm_configure(self, slots: int):
        """Allocate and zero the state machine with `slots` registers per
        replica (a power of two in 1..64; again: zero it or resize it); 0 frees it."""
        slots = _int("sm_configure", "slots", slots, want="0 or a power of two in 1..64")
        if slots != 0 and slots not in abi.SM_SLOTS:
            raise ValueError(f"sm_configure: slots must be 0 or a power of two in 1..64, not {slots!r}")
        self._check(self._lib.raft_engine_sm_configure(self._h, slots), "sm_configure")
        self._sm_slots = slots

    def sm_apply(self, g0: int = 0, n: int | None = None, replica: int = -1) -> dict:
        """Apply the entries of groups [g0, g0 + n) (replica -1: every replica,
        else that replica index) that became committed since each machine's
        cursor, on the device: info with applied, lost, regressed, status.
        RAFT_EWINDOW (entries left the log window unapplied) is not raised: the
        call did everything else and info["status"] carries the code."""
        g0, n, replica = self._replica_span(g0, n, replica, "sm_apply")
        si = abi.raft_sm_info()
        rc = self._lib.raft_engine_sm_apply(self._h, g0, n, replica, C.byref(si))
        if rc != abi.RAFT_EWINDOW:
            self._check(rc, "sm_apply")
        return {**abi.info_dict(si), "status": int(rc)}

    def sm_read(self, g0: int = 0, n: int | None = None, regs: bool = True):
        """The machines of groups [g0, g0 + n): (heads, regs) -- heads [n, R] of
        abi.SM_HEAD_DTYPE (applied, lost, hash), regs [n, R, slots] uint32 (None
        with regs=False)."""
        n = self.G - g0 if n is None else n
        h = np.zeros((max(int(n), 0), self.R), dtype=abi.SM_HEAD_DTYPE)   # a bad range is the library's to refuse
        r = np.zeros((max(int(n), 0), self.R, self.sm_slots), dtype=np.uint32) if regs and self.sm_slots else None
        self._check(self._lib.raft_engine_sm_read(self._h, int(g0), int(n), C.c_void_p(h.ctypes.data),
                                                  C.c_void_p(r.ctypes.data) if r is not None else None), "sm_read")
        return h, r

    def sm_write(self, heads=None, regs=None, g0: int = 0):
        """Store the machines of groups [g0, g0 + n) (resuming a run): heads
        [n, R] of abi.SM_HEAD_DTYPE with applied in 0..log_cap and lost >= 0,
        regs an integer [n, R, slots] array; either may be None."""
        if heads is None and regs is None:
            raise ValueError("sm_write: heads or regs is required")
        n = None
        if heads is not None:
            heads = np.ascontiguousarray(heads)
            if heads.dtype != abi.SM_HEAD_DTYPE or heads.ndim != 2 or heads.shape[1] != self.R:
                raise ValueError(f"sm_write: heads must be abi.SM_HEAD_DTYPE records of shape (n, {self.R})")
            if heads.size and (heads["applied"].min() < 0 or heads["applied"].max() > self.cap or heads["lost"].min() < 0):
                raise ValueError(f"sm_write: every applied must be in 0..{self.cap} and every lost >= 0")
            n = heads.shape[0]
        if regs is not None:
            regs = np.asarray(regs)
            if regs.ndim != 3 or regs.shape[1:] != (self.R, self.sm_slots) or regs.dtype.kind not in "iu":
                raise ValueError(f"sm_write: regs {regs.shape} {regs.dtype} must be an integer array of shape "
                                 f"(n, {self.R}, {self.sm_slots})")
            if n is not None and regs.shape[0] != n:
                raise ValueError(f"sm_write: heads hold {n} groups and regs {regs.shape[0]}")
            n = regs.shape[0]
            regs = np.ascontiguousarray(regs, dtype=np.uint32)
        self._check(self._lib.raft_engine_sm_write(self._h, int(g0), n,
                                                   C.c_void_p(heads.ctypes.data) if heads is not None else None,
                                                   C.c_void_p(regs.ctypes.data) if regs is not None else None), "sm_write")

    def sm_get(self, groups, keys, replica=-1) -> np.ndarray:
        """The batched client read: register keys[m] (its low bits name the
        slot) of groups[m], from `replica` (one index for all, or one per
        request; -1: the group's leader).  Returns abi.SM_VALUE_DTYPE records:
        value, the replica read (-1 and value 0 without a leader), its applied
        cursor and its commitIndex."""
        g, k = self._client_arrays(groups, keys, "sm_get")
        r = np.asarray(replica)
        if r.ndim == 0:
            r = np.full(g.shape, r)
        if r.dtype.kind not in "iu" or r.shape != g.shape:
            raise ValueError(f"sm_get: replica must be an integer or {g.shape[0]} integers")
        if r.size and (r.min() < -1 or r.max() >= self.R):
            raise ValueError(f"sm_get: every replica must be -1 (the leader) or in 0..{self.R - 1}")
        r = np.ascontiguousarray(r, dtype=np.int32)
        out = np.zeros(g.shape[0], dtype=abi.SM_VALUE_DTYPE)
        self._check(self._lib.raft_engine_sm_get(self._h, C.c_void_p(g.ctypes.data), C.c_void_p(r.ctypes.data),
                                                 C.c_void_p(k.ctypes.data), C.c_void_p(out.ctypes.data), g.shape[0]),
                    "sm_get")
        return out

    def sm_check(self, g0: int = 0, n: int | None = None, flags: bool = False):
        """State Machine Safety: groups with two replicas that lost nothing,
        applied equally many entries and hold different hashes; returns the
        count, or (count, per-group uint8 flags) with flags=True."""
        n = self.G - g0 if n is None else n
        f = np.zeros(max(int(n), 0), dtype=np.uint8) if flags else None
        out = C.c_int64()
        self._check(self._lib.raft_engine_sm_check(self._h, int(g0), int(n), abi.ptr(f, C.c_uint8) if flags else None,
                                                   C.byref(out)), "sm_check")
        return (int(out.value), f) if flags else int(out.value)

    # -- replica crash and restart (raft_engine_restart*) -------------------------
    def _restart_args(self, g0, n, amnesia, replay, down_steps, what: str):
        """The arguments every restart form shares, checked before any library call."""
        g0, n = _span(what, self.G, g0, n)
        down_steps = _int(what, "down_steps", down_steps, 0, abi.RESTART_MAX_DOWN_STEPS)
        flags = (abi.RESTART_AMNESIA if amnesia else 0) | (abi.RESTART_REPLAY if replay else 0)
        return g0, n, flags, down_steps

    def restart(self, mask=None, *, ppm: int | None = None, g0: int = 0, n: int | None = None,
                amnesia: bool = False, replay: bool = False, down_steps: int = 0) -> dict:
        """Crash and restart replicas of groups [g0, g0 + n) on the device: they
        come back as FOLLOWERs with commitIndex 0, no election or heartbeat
        session and a fresh election timeout.  Exactly one of `mask` (n bytes,
        bit r of mask[j]: replica r of group g0 + j) and `ppm` (a seeded rate per
        replica, drawn at the current step index) selects them.  By default
        currentTerm, votedFor and the log are kept and so are lastApplied and
        the machine; replay=True also zeroes those consumers; amnesia=True also
        forgets term, vote and log.  down_steps > 0 isolates the lowest
        restarted replica of each group for that many steps (the harness's
        isolation: cut off, timers running).  Returns restarted, leaders,
        entries_dropped (include/raft_engine.h raft_restart_info)."""
        if (mask is None) == (ppm is None):
            raise ValueError("restart: exactly one of mask and ppm is required")
        if mask is not None:
            m, n = self._byte_mask(mask, n, "restart")
        else:
            ppm = _int("restart", "ppm", ppm, 0, 0xFFFFFFFF)
        g0, n, flags, down_steps = self._restart_args(g0, n, amnesia, replay, down_steps, "restart")
        ri = abi.raft_restart_info()
        if mask is not None:
            rc = self._lib.raft_engine_restart(self._h, g0, n, C.c_void_p(m.ctypes.data), flags, down_steps, C.byref(ri))
        else:
            rc = self._lib.raft_engine_restart_random(self._h, g0, n, ppm, flags, down_steps, C.byref(ri))
        self._check(rc, "raft_engine_restart" if mask is not None else "raft_engine_restart_random")
        return abi.info_dict(ri)

    def restart_dev(self, mask_ptr: int, *, g0: int = 0, n: int | None = None, amnesia: bool = False,
                    replay: bool = False, down_steps: int = 0, after_stream: int | None = None) -> dict:
        """restart with the mask in DEVICE memory (n bytes on this engine's GPU,
        e.g. a torch uint8 tensor's data_ptr()); returns once the kernel finished."""
        g0, n, flags, down_steps = self._restart_args(g0, n, amnesia, replay, down_steps, "restart_dev")
        if n > 0 and not mask_ptr:
            raise ValueError("restart_dev: a device mask is required")
        self._dev("restart_dev", after_stream)
        ri = abi.raft_restart_info()
        self._check(self._lib.raft_engine_restart_dev(self._h, g0, n, C.c_void_p(mask_ptr or 0), flags, down_steps,
                                                      C.byref(ri)), "raft_engine_restart_dev")
        return abi.info_dict(ri)

    # -- snapshot install (raft_engine_install_snapshot*) --------------------------
    def install_snapshot(self, mask=None, *, g0: int = 0, n: int | None = None, min_lag: int = 0,
                         device_mask: int | None = None) -> dict:
        """Heal lagging replicas of groups [g0, g0 + n) from their group's newest
        leader, on the device (engine.sm_configure first): an eligible replica
        whose lastIndex is at least `min_lag` behind the leader's and whose term
        is not above it gets the leader's retained log, commit point, term and
        machine, comes back as a FOLLOWER with a fresh election timeout, and the
        leader's session counts it as caught up.  `mask` (n bytes, bit r of
        mask[j]: replica r of group g0 + j) or `device_mask` (the same bytes in
        DEVICE memory, e.g. a torch uint8 tensor's data_ptr()) names the
        eligible replicas; neither: every replica.  Returns installed,
        slots_copied, no_leader, leader_gapped, ahead (include/raft_engine.h
        raft_install_info)."""
        if mask is not None and device_mask is not None:
            raise ValueError("install_snapshot: at most one of mask and device_mask")
        m = None
        if mask is not None:
            m, n = self._byte_mask(mask, n, "install_snapshot")
        g0, n = _span("install_snapshot", self.G, g0, n)
        min_lag = _int("install_snapshot", "min_lag", min_lag, 0)
        ii = abi.raft_install_info()
        if device_mask is not None:
            rc = self._lib.raft_engine_install_snapshot_dev(self._h, g0, n, C.c_void_p(int(device_mask)), min_lag,
                                                            C.byref(ii))
        else:
            rc = self._lib.raft_engine_install_snapshot(self._h, g0, n,
                                                        C.c_void_p(m.ctypes.data) if m is not None and m.size else None,
                                                        min_lag, C.byref(ii))
        self._check(rc, "raft_engine_install_snapshot")
        return abi.info_dict(ii)

    # -- leadership transfer (raft_transfer_batch*, raft_engine_resolve_transfers*, raft_engine_evacuate*) ----
    def transfer(self, groups, targets=None) -> np.ndarray:
        """raft_transfer_batch: ask groups[m] to move its leadership to replica
        targets[m] (abi.TRANSFER_AUTO, or targets=None: the first caught-up idle
        follower after the leader, cyclically).  The target's election timer is
        set to fire in the next step; nothing else is written.  Returns
        abi.TRANSFER_TICKET_DTYPE tickets (from: the group's newest leader, its
        term, target, status = abi.TRANSFER_SENT ... TRANSFER_INVALID)."""
        g = np.ascontiguousarray(groups, dtype=np.int64)
        t = np.full(g.shape, abi.TRANSFER_AUTO, dtype=np.int32) if targets is None else \
            np.ascontiguousarray(targets, dtype=np.int32)
        if g.ndim != 1 or t.shape != g.shape:
            raise ValueError(f"transfer: groups {g.shape} and targets {t.shape} must be 1-D and of one length")
        tk = np.zeros(g.shape[0], dtype=abi.TRANSFER_TICKET_DTYPE)
        self._check(self._lib.raft_transfer_batch(self._h, C.c_void_p(g.ctypes.data), C.c_void_p(t.ctypes.data),
                                                  C.c_void_p(tk.ctypes.data), g.shape[0]), "raft_transfer_batch")
        return tk

    def transfer_dev(self, group_ptr: int, target_ptr: int, ticket_ptr: int, n: int,
                     after_stream: int | None = None) -> int:
        """raft_transfer_batch_dev: DEVICE pointers to n int64 groups, int32
        targets and 16-byte tickets (16-byte aligned), e.g. torch tensors'
        data_ptr(); returns RAFT_OK once the batch finished."""
        self._dev("transfer_dev", after_stream, ticket=ticket_ptr)
        return self._client_status(self._lib.raft_transfer_batch_dev(self._h, group_ptr, target_ptr, ticket_ptr, int(n)),
                                   "raft_transfer_batch_dev", ())

    def resolve_transfers(self, groups, tickets, check: bool = True) -> np.ndarray:
        """raft_engine_resolve_transfers: what became of each transfer ticket, as
        abi.TRANSFER_STATE_DTYPE records (status = abi.TRANSFER_COMPLETED /
        TRANSFER_PENDING / TRANSFER_SUPERSEDED / TRANSFER_NONE / TRANSFER_INVALID,
        the leader found and its term).  Read-only.  With check=False
        RAFT_ERANGE / RAFT_EINVAL (some record is INVALID) are not raised:
        ``last_status`` carries the code."""
        g = np.ascontiguousarray(groups, dtype=np.int64)
        t = np.ascontiguousarray(tickets)
        if g.ndim != 1 or t.dtype != abi.TRANSFER_TICKET_DTYPE or t.ndim != 1 or t.shape[0] != g.shape[0]:
            raise ValueError(f"resolve_transfers: tickets must be {g.shape[0]} records of abi.TRANSFER_TICKET_DTYPE")
        out = np.zeros(g.shape[0], dtype=abi.TRANSFER_STATE_DTYPE)
        self._client_status(self._lib.raft_engine_resolve_transfers(
            self._h, C.c_void_p(g.ctypes.data), C.c_void_p(t.ctypes.data), C.c_void_p(out.ctypes.data), g.shape[0]),
            "raft_engine_resolve_transfers", () if check else (abi.RAFT_ERANGE, abi.RAFT_EINVAL))
        return out

    def resolve_transfers_dev(self, group_ptr: int, ticket_ptr: int, out_ptr: int, n: int,
                              after_stream: int | None = None, check: bool = True) -> int:
        """raft_engine_resolve_transfers_dev on DEVICE pointers (tickets and
        records 16-byte aligned); returns the call's code (see resolve_transfers)."""
        self._dev("resolve_transfers_dev", after_stream, ticket=ticket_ptr, record=out_ptr)
        return self._client_status(self._lib.raft_engine_resolve_transfers_dev(self._h, group_ptr, ticket_ptr, out_ptr,
                                                                               int(n)),
                                   "raft_engine_resolve_transfers_dev", () if check else (abi.RAFT_ERANGE, abi.RAFT_EINVAL))

    def evacuate(self, mask, g0: int = 0) -> dict:
        """raft_engine_evacuate: for every group of [g0, g0 + len(mask)) whose
        newest leader has its bit set in mask[j] (bit r: replica r), fire the
        election timer of the first caught-up idle follower outside the mask
        after that leader, cyclically -- the step before a planned restart of
        the masked replicas.  Returns led, sent, no_target, behind, busy
        (include/raft_engine.h raft_evacuate_info)."""
        m, n = self._byte_mask(mask, None, "evacuate")
        g0 = _int("evacuate", "g0", g0)
        ei = abi.raft_evacuate_info()
        self._check(self._lib.raft_engine_evacuate(self._h, g0, n, C.c_void_p(m.ctypes.data) if m.size else None,
                                                   C.byref(ei)), "raft_engine_evacuate")
        return abi.info_dict(ei)

    def evacuate_dev(self, mask_ptr: int, n: int, g0: int = 0, after_stream: int | None = None) -> dict:
        """evacuate with the mask in DEVICE memory (n bytes on this engine's GPU,
        e.g. a torch uint8 tensor's data_ptr()); returns once the kernel finished."""
        if n > 0 and not mask_ptr:
            raise ValueError("evacuate_dev: a device mask is required")
        self._dev("evacuate_dev", after_stream)
        ei = abi.raft_evacuate_info()
        self._check(self._lib.raft_engine_evacuate_dev(self._h, int(g0), int(n), C.c_void_p(mask_ptr or 0), C.byref(ei)),
                    "raft_engine_evacuate_dev")
        return abi.info_dict(ei)

    # -- scripted network faults (raft_isolate_batch*, raft_engine_heal_network*, raft_engine_list_isolated*) ----
    def isolate(self, groups, targets, steps, replace: bool = False) -> np.ndarray:
        """raft_isolate_batch: cut replica targets[m] of groups[m] off from its
        group for steps[m] (the group's isolation word becomes steps << 8 |
        replica: it cuts the next steps - 1 steps).  A target is a replica
        index, abi.ISOLATE_NEWEST_LEADER or abi.ISOLATE_LOWEST_LEADER; targets
        and steps may be scalars.  Per group only the first message of the
        batch is judged; a running isolation is kept (BUSY) unless
        replace=True.  Returns abi.ISOLATE_TICKET_DTYPE tickets (replica, steps,
        status = abi.ISOLATE_SET ... ISOLATE_INVALID, prev: the word found, or
        for DUPLICATE the judged message's position)."""
        g = np.ascontiguousarray(groups, dtype=np.int64)
        if g.ndim != 1:
            raise ValueError(f"isolate: groups {g.shape} must be 1-D")
        t, s = np.asarray(targets), np.asarray(steps)
        for name, a in (("targets", t), ("steps", s)):
            if a.ndim > 1 or (a.ndim == 1 and a.shape != g.shape) or (
                    a.size and (a.dtype.kind not in "iu" or a.min() < -0x80000000 or a.max() > 0x7FFFFFFF)):
                raise ValueError(f"isolate: {name} must be an int32 scalar or one per group, not {a.shape} {a.dtype}")
        t = np.ascontiguousarray(np.broadcast_to(t, g.shape), dtype=np.int32)
        s = np.ascontiguousarray(np.broadcast_to(s, g.shape), dtype=np.int32)
        tk = np.zeros(g.shape[0], dtype=abi.ISOLATE_TICKET_DTYPE)
        self._check(self._lib.raft_isolate_batch(
            self._h, C.c_void_p(g.ctypes.data), C.c_void_p(t.ctypes.data), C.c_void_p(s.ctypes.data),
            abi.ISOLATE_REPLACE if replace else 0, C.c_void_p(tk.ctypes.data), g.shape[0]), "raft_isolate_batch")
        return tk

    def isolate_dev(self, group_ptr: int, target_ptr: int, steps_ptr: int, ticket_ptr: int, n: int,
                    replace: bool = False, after_stream: int | None = None) -> int:
        """raft_isolate_batch_dev: DEVICE pointers to n int64 groups, int32
        targets, int32 steps and 16-byte tickets (16-byte aligned), e.g. torch
        tensors' data_ptr(); returns RAFT_OK once the batch finished."""
        self._dev("isolate_dev", after_stream, ticket=ticket_ptr)
        return self._client_status(self._lib.raft_isolate_batch_dev(
            self._h, group_ptr, target_ptr, steps_ptr, abi.ISOLATE_REPLACE if replace else 0, ticket_ptr, int(n)),
            "raft_isolate_batch_dev", ())

    def heal_network(self, mask=None, g0: int = 0, n: int | None = None) -> dict:
        """raft_engine_heal_network: clear the running isolation word of every
        group of [g0, g0 + n) whose isolated replica r has bit r set in mask[j]
        (mask=None: whichever replica it is) -- the state the step kernel's own
        expiry leaves.  Returns healed, idle (nothing was running), kept
        (running, not selected)."""
        m = None
        if mask is not None:
            m, n = self._byte_mask(mask, n, "heal_network")
        g0, n = _span("heal_network", self.G, g0, n)
        hi = abi.raft_heal_info()
        self._check(self._lib.raft_engine_heal_network(self._h, g0, n,
                                                       C.c_void_p(m.ctypes.data) if m is not None and m.size else None,
                                                       C.byref(hi)), "raft_engine_heal_network")
        return abi.info_dict(hi)

    def heal_network_dev(self, mask_ptr: int, n: int, g0: int = 0, after_stream: int | None = None) -> dict:
        """heal_network with the mask in DEVICE memory (n bytes on this engine's
        GPU, e.g. a torch uint8 tensor's data_ptr(); 0: any replica); returns
        once the kernel finished."""
        self._dev("heal_network_dev", after_stream)
        hi = abi.raft_heal_info()
        self._check(self._lib.raft_engine_heal_network_dev(self._h, int(g0), int(n), C.c_void_p(mask_ptr or 0),
                                                           C.byref(hi)), "raft_engine_heal_network_dev")
        return abi.info_dict(hi)

    def isolated(self, g0: int = 0, n: int | None = None, max_events: int | None = None, peek: bool = False):
        """raft_engine_list_isolated: the groups of [g0, g0 + n) with a running
        isolation: (info, records).  records is a numpy array of
        abi.ISOLATED_DTYPE (group, replica, role of that replica now, remaining)
        in ascending group order, at most max_events of them (None: as many as
        there are).  peek=True returns no record.  info: delivered, pending,
        running.  Read-only."""
        call = _stream_call(self, "raft_engine_list_isolated", *_span("isolated", self.G, g0, n))
        return _ISOLATED.host(self._check, "isolated", call, max_events, peek)

    def isolated_dev(self, out_ptr: int, max_events: int, g0: int = 0, n: int | None = None,
                     after_stream: int | None = None) -> dict:
        """isolated into a DEVICE buffer of max_events 16-byte records (16-byte
        aligned); returns the info once the kernels finished."""
        return self._records_dev(_ISOLATED, "isolated_dev", "raft_engine_list_isolated_dev",
                                 _span("isolated_dev", self.G, g0, n), out_ptr, max_events, after_stream)

    # -- leader no-op entries (raft_engine_append_noops*, raft_engine_sm_set_noop) -------------------------
    def _noop_args(self, g0, n, cmd, what: str):
        return (*_span(what, self.G, g0, n), _int(what, "cmd", cmd, 0, 0xFFFFFFFF, want="a u32 command id"))

    def append_noops(self, g0: int = 0, n: int | None = None, cmd: int = abi.NOOP_CMD, tickets: bool = False):
        """raft_engine_append_noops: in every group of [g0, g0 + n) whose newest
        leader's last entry is not of its own term (or whose log is empty),
        appendCommand of `cmd` on that leader -- Raft's no-op entry, after which
        the leader can commit what earlier terms left and serve linearizable
        reads.  A second call in the same term appends nothing.  Returns the
        info (appended, current, no_leader, log_full, ghosted; include/raft_engine.h
        raft_noop_info), or with tickets=True (info, tickets, cmds): per group an
        abi.TICKET_DTYPE ticket (status abi.PROPOSE_CURRENT where nothing was
        appended: it names the leader's last entry) and the command id to
        resolve it with.  RAFT_EWINDOW (a textbook add below a log_window) is not
        raised: ``last_status`` carries the code."""
        g0, n, cmd = self._noop_args(g0, n, cmd, "append_noops")
        ni = abi.raft_noop_info()
        t = np.zeros(max(n, 0), dtype=abi.TICKET_DTYPE) if tickets else None    # a bad range is the library's to refuse
        c = np.zeros(max(n, 0), dtype=np.uint32) if tickets else None
        self._client_status(self._lib.raft_engine_append_noops(
            self._h, g0, n, cmd, C.c_void_p(t.ctypes.data) if tickets else None,
            C.c_void_p(c.ctypes.data) if tickets else None, C.byref(ni)), "raft_engine_append_noops")
        info = abi.info_dict(ni)
        return (info, t, c) if tickets else info

    def append_noops_dev(self, ticket_ptr: int, cmd_ptr: int, g0: int = 0, n: int | None = None,
                         cmd: int = abi.NOOP_CMD, after_stream: int | None = None) -> dict:
        """append_noops with the tickets ([n] 16-byte records, 16-byte aligned)
        and their command ids ([n] uint32) written to DEVICE memory, or both
        pointers 0 for none; returns the info once the kernel finished."""
        g0, n, cmd = self._noop_args(g0, n, cmd, "append_noops_dev")
        self._dev("append_noops_dev", after_stream, ticket=ticket_ptr)
        ni = abi.raft_noop_info()
        self._client_status(self._lib.raft_engine_append_noops_dev(
            self._h, g0, n, cmd, C.c_void_p(ticket_ptr or 0), C.c_void_p(cmd_ptr or 0), C.byref(ni)),
            "raft_engine_append_noops_dev")
        return abi.info_dict(ni)

    def sm_set_noop(self, cmd: int | None = abi.NOOP_CMD):
        """raft_engine_sm_set_noop: from now on sm_apply counts and hashes an
        entry whose command id is `cmd` like any other and writes no register
        for it; cmd=None switches that off (the default).  The setting is the
        engine's: it may be made before sm_configure and outlives reset."""
        cmd = _int("sm_set_noop", "cmd", cmd, 0, 0xFFFFFFFF, allow_none=True, want="a u32 command id")
        self._check(self._lib.raft_engine_sm_set_noop(self._h, int(cmd is not None), cmd or 0), "sm_set_noop")

    # -- the leader watch (raft_engine_poll_leaders*, raft_engine_read_watch / write_watch) -----------------
    def poll_leaders(self, g0: int = 0, n: int | None = None, max_events: int | None = None, peek: bool = False):
        """raft_engine_poll_leaders: the groups of [g0, g0 + n) whose newest
        leader (role LEADER, the highest currentTerm, the lowest index among
        equals) or its term changed since the watch last reported them:
        (info, events).  events is a numpy array of abi.EVENT_DTYPE (group,
        leader, term, prev_leader, prev_term; -1 and 0 where there is none) in
        ascending group order, at most max_events of them (None: as many as
        there are -- a peek sizes the buffer); the watch advances for the
        groups that were returned.  peek=True stores nothing and returns no
        event.  info: delivered, pending, and over the whole range gained,
        lost, moved, reterm, leaderless (include/raft_engine.h raft_watch_info)."""
        call = _stream_call(self, "raft_engine_poll_leaders", *_span("poll_leaders", self.G, g0, n))
        return _WATCH.host(self._check, "poll_leaders", call, max_events, peek)

    def poll_leaders_dev(self, out_ptr: int, max_events: int, g0: int = 0, n: int | None = None,
                         after_stream: int | None = None) -> dict:
        """poll_leaders into a DEVICE buffer of max_events 24-byte records (8-byte
        aligned); returns the info once the kernels finished."""
        return self._records_dev(_WATCH, "poll_leaders_dev", "raft_engine_poll_leaders_dev",
                                 _span("poll_leaders_dev", self.G, g0, n), out_ptr, max_events, after_stream)

    def read_watch(self, g0: int = 0, n: int | None = None) -> np.ndarray:
        """What the watch last reported for groups [g0, g0 + n): [n, 2] int32
        (leader, term), (-1, 0) before the first report."""
        n = self.G - g0 if n is None else n
        out = np.zeros((max(int(n), 0), 2), dtype=np.int32)           # a bad range is the library's to refuse
        self._check(self._lib.raft_engine_read_watch(self._h, int(g0), int(n), abi.ptr(out, C.c_int32)), "read_watch")
        return out

    def write_watch(self, seen: np.ndarray, g0: int = 0):
        """Store the watch's pairs of groups [g0, g0 + len(seen)) (resuming a
        consumer): an integer [n, 2] array of (leader in -1..R-1, term >= 0),
        a leader of -1 with term 0 only."""
        a = np.asarray(seen)
        if a.ndim != 2 or a.shape[1] != 2 or a.dtype.kind not in "iu":
            raise ValueError(f"write_watch: seen {a.shape} {a.dtype} must be an integer array of shape (n, 2)")
        if a.size and (a[:, 0].min() < -1 or a[:, 0].max() >= self.R or a[:, 1].min() < 0
                       or a[:, 1].max() > 0x7FFFFFFF or (a[a[:, 0] < 0, 1] != 0).any()):
            raise ValueError(f"write_watch: every pair must be (-1, 0) or (leader in 0..{self.R - 1}, term >= 0)")
        a = np.ascontiguousarray(a, dtype=np.int32)
        self._check(self._lib.raft_engine_write_watch(self._h, int(g0), a.shape[0], abi.ptr(a, C.c_int32)), "write_watch")

    # -- the safety audit (raft_audit_*) ----------------------------------------------------------------
    def audit(self) -> RaftAudit:
        """A new safety audit of this engine, every ledger in its zero state
        (RaftAudit: observe, report, read, write, reset, close).  Closing the
        engine closes its audits first."""
        return self._adopt(RaftAudit(self))

    # -- the liveness monitor (raft_monitor_*) ------------------------------------------------------------
    def monitor(self, leaderless_steps: int = 0, stalled_steps: int = abi.MONITOR_STALLED_STEPS, lag_entries: int = 0,
                churn_terms: int = 0, churn_steps: int = 1) -> RaftMonitor:
        """A new liveness monitor of this engine, every ledger in its zero state
        (RaftMonitor: observe, report, report_dev, read, write, reset,
        availability, set_availability, device_bytes, close).  A group is
        LEADERLESS once it has shown no leader for leaderless_steps steps,
        COMMIT_STALLED once its leader's backlog has not advanced for
        stalled_steps, LAGGING while a replica is lag_entries or more behind the
        newest leader (0: off), CHURNING when its highest term rose by
        churn_terms within a window of churn_steps (0: off).  Closing the engine
        closes its monitors first."""
        return self._adopt(RaftMonitor(self, leaderless_steps=leaderless_steps, stalled_steps=stalled_steps,
                                       lag_entries=lag_entries, churn_terms=churn_terms, churn_steps=churn_steps))

    # -- the persistence stream (raft_wal_*) ------------------------------------------------------------
    def wal(self) -> RaftWal:
        """A new persistence stream of this engine, every cursor fresh (RaftWal:
        poll, poll_dev, peek, cursors, set_cursors, reset, device_bytes, close):
        the first poll hands out every replica's hard state and whole log, the
        later ones what changed.  Closing the engine closes its streams first."""
        return self._adopt(RaftWal(self))

    # -- the proposal outbox (raft_engine_outbox_*, raft_outbox_submit*) ---------------------------------
    def outbox_configure(self, capacity: int, expire_steps: int = 0):
        """raft_engine_outbox_configure: a queue of `capacity` proposals in HBM;
        a record older than expire_steps steps completes EXPIRED (0: never)."""
        capacity = _int("outbox_configure", "capacity", capacity, 1, 2 ** 31 - 1)
        expire_steps = _int("outbox_configure", "expire_steps", expire_steps, 0, 2 ** 31 - 1)
        self._check(self._lib.raft_engine_outbox_configure(self._h, capacity, expire_steps), "outbox_configure")

    def outbox_submit(self, groups, cmds, tags):
        """raft_outbox_submit: enqueue proposal cmds[m] (a u32 id) for groups[m]
        under the caller's tags[m] (int64), in batch order.  Nothing is proposed
        before the next outbox_pump.  RAFT_EFULL / RAFT_ERANGE raise RaftError
        and enqueue nothing."""
        g, c = self._client_arrays(groups, cmds, "outbox_submit")
        t = np.ascontiguousarray(tags, dtype=np.int64)
        if t.ndim != 1 or t.shape[0] != g.shape[0]:
            raise ValueError(f"outbox_submit: tags {t.shape} must be 1-D and as long as groups")
        self._check(self._lib.raft_outbox_submit(self._h, C.c_void_p(g.ctypes.data), C.c_void_p(c.ctypes.data),
                                                 C.c_void_p(t.ctypes.data), g.shape[0]), "raft_outbox_submit")

    def outbox_submit_dev(self, group_ptr: int, cmd_ptr: int, tag_ptr: int, n: int, after_stream: int | None = None):
        """raft_outbox_submit_dev: DEVICE pointers to n int64 groups, uint32
        commands and int64 tags."""
        self._dev("outbox_submit_dev", after_stream)
        self._check(self._lib.raft_outbox_submit_dev(self._h, group_ptr, cmd_ptr, tag_ptr, int(n)),
                    "raft_outbox_submit_dev")

    @staticmethod
    def _outbox_info(info) -> dict:
        return {**abi.info_dict(info), "age_hist": [int(x) for x in info.age_hist]}

    def outbox_len(self) -> int:
        """Records in the outbox now (raft_engine_outbox_read's peek)."""
        n = C.c_int64()
        self._check(self._lib.raft_engine_outbox_read(self._h, None, 0, C.byref(n)), "outbox_read")
        return int(n.value)

    def outbox_pump(self, max_done: int | None = None):
        """raft_engine_outbox_pump: every record gets its verdict from the
        state the call finds; the COMMITTED and EXPIRED ones (the first
        max_done in queue order; None: all of them) are returned as
        abi.OUTBOX_DONE_DTYPE records and leave the queue, the ones no replica
        holds any more are proposed again, the rest stay.  Returns (info,
        records): info has abi.OUTBOX_INFO_FIELDS and age_hist (32 buckets).
        RAFT_EWINDOW (a record UNKNOWN below a log_window, or a retried add
        below one) is not raised: ``last_status`` carries the code."""
        max_done = _int("outbox_pump", "max_done", self.outbox_len() if max_done is None else max_done, 0)
        out = np.zeros(max_done, dtype=abi.OUTBOX_DONE_DTYPE)
        n, info = C.c_int64(), abi.raft_outbox_info()
        self._client_status(self._lib.raft_engine_outbox_pump(self._h, C.c_void_p(out.ctypes.data) if max_done else None,
                                                              max_done, C.byref(n), C.byref(info)),
                            "raft_engine_outbox_pump")
        return self._outbox_info(info), out[: int(n.value)]

    def outbox_pump_dev(self, done_ptr: int, max_done: int, after_stream: int | None = None):
        """outbox_pump into a DEVICE buffer of max_done 32-byte records (16-byte
        aligned); returns (info, records written)."""
        self._dev("outbox_pump_dev", after_stream, record=done_ptr)
        n, info = C.c_int64(), abi.raft_outbox_info()
        self._client_status(self._lib.raft_engine_outbox_pump_dev(self._h, C.c_void_p(done_ptr), int(max_done),
                                                                  C.byref(n), C.byref(info)),
                            "raft_engine_outbox_pump_dev")
        return self._outbox_info(info), int(n.value)

    def outbox_read(self) -> np.ndarray:
        """The queue in order, as abi.OUTBOX_ENTRY_DTYPE records."""
        out = np.zeros(self.outbox_len(), dtype=abi.OUTBOX_ENTRY_DTYPE)
        n = C.c_int64()
        if len(out):
            self._check(self._lib.raft_engine_outbox_read(self._h, C.c_void_p(out.ctypes.data), len(out), C.byref(n)),
                        "outbox_read")
        return out

    def outbox_write(self, records: np.ndarray):
        """Replace the queue with `records` (abi.OUTBOX_ENTRY_DTYPE; resuming an
        outbox_read).  The library refuses, before storing anything, a group,
        replica, index or status a pump would not accept."""
        a = np.ascontiguousarray(records)
        if a.dtype != abi.OUTBOX_ENTRY_DTYPE or a.ndim != 1:
            raise ValueError("outbox_write: records must be a 1-D array of abi.OUTBOX_ENTRY_DTYPE")
        self._check(self._lib.raft_engine_outbox_write(self._h, C.c_void_p(a.ctypes.data) if len(a) else None, len(a)),
                    "outbox_write")

    def allreduce_counters(self, comm: RaftComm, counters_ptr: int, out_ptr: int, n_steps: int):
        """raft_engine_allreduce_counters: the sum over the ranks of n_steps
        counter rows (DEVICE pointers, [n_steps][COUNTER_STRIDE] int64; in
        place when out_ptr == counters_ptr), enqueued on the engine stream
        after its step launches."""
        self._check(self._lib.raft_engine_allreduce_counters(self._h, comm._h, C.c_void_p(counters_ptr),
                                                             C.c_void_p(out_ptr), int(n_steps)),
                    "raft_engine_allreduce_counters")

    def timed_span(self, end_event_ptr: int) -> float:
        """raft_engine_timed_span: ms from the first timed step launch's start to
        the caller's event (e.g. torch.cuda.Event.cuda_event); call before
        kernel_time()."""
        ms = C.c_double()
        self._check(self._lib.raft_engine_timed_span(self._h, C.c_void_p(end_event_ptr), C.byref(ms)), "timed_span")
        return float(ms.value)

    def traffic_probe(self, kind: int) -> tuple[int, int]:
        """raft_engine_traffic_probe: one dispatch of the step kernel's own HBM
        access pattern (kind 0: the state into registers and back; kind 1: one
        8-byte log store per replica, flat logs only); returns (bytes read,
        bytes written) for calibrating rocprofv3's FETCH_SIZE / WRITE_SIZE."""
        r, w = C.c_int64(), C.c_int64()
        self._check(self._lib.raft_engine_traffic_probe(self._h, int(kind), C.byref(r), C.byref(w)), "traffic_probe")
        return int(r.value), int(w.value)

    # -- the service boundary (RaftServer.kt:228-287, :100-107) -------------
    @staticmethod
    def _batch_index(group, dst, n: int, what: str):
        """group / dst as contiguous int64 / int32 vectors of exactly n entries
        (the C side reads n of each)."""
        g = np.ascontiguousarray(group, dtype=np.int64)
        d = np.ascontiguousarray(dst, dtype=np.int32)
        if g.ndim != 1 or d.ndim != 1 or g.shape[0] != n or d.shape[0] != n:
            raise ValueError(f"{what}: group {g.shape} and replica {d.shape} must be 1-D with {n} entries")
        return g, d

    @staticmethod
    def _batch_out(out, n: int, w: int, what: str) -> np.ndarray:
        """The response array: a new [n, w] int32 array, or the caller's (e.g. a
        view of page-locked memory, which the engine's DMA writes directly)."""
        if out is None:
            return np.zeros((n, w), dtype=np.int32)
        if out.dtype != np.int32 or out.shape != (n, w) or not out.flags.c_contiguous:
            raise ValueError(f"{what}: out must be a C-contiguous int32 array of shape {(n, w)}")
        return out

    def vote_batch(self, group, dst, req: np.ndarray, out: np.ndarray | None = None) -> np.ndarray:
        """req: [n, 4] int32 (term, candidateId, lastLogIndex, lastLogTerm) ->
        [n, 2] int32 (term, voteGranted), into `out` when given.  Page-locked
        arrays (all four) are moved by DMA with no staging copy."""
        q = np.ascontiguousarray(req, dtype=np.int32).reshape(-1, 4)
        g, d = self._batch_index(group, dst, q.shape[0], "vote_batch")
        out = self._batch_out(out, q.shape[0], 2, "vote_batch")
        self._check(self._lib.raft_vote_batch(self._h, abi.ptr(g, C.c_int64), abi.ptr(d, C.c_int32),
                                              abi.ptr(q, abi.raft_vote_req), abi.ptr(out, abi.raft_vote_resp),
                                              q.shape[0]), "raft_vote_batch")
        return out

    def append_batch(self, group, dst, req: np.ndarray, out: np.ndarray | None = None) -> np.ndarray:
        """req: [n, 8] int32 (term, leaderId, prevLogIndex, prevLogTerm, hasEntry,
        entryTerm, entryCmd(u32 bits), leaderCommit) -> [n, 3] (term, success, status),
        into `out` when given."""
        req = np.asarray(req)
        if req.dtype == np.int32 or req.dtype == np.uint32:       # already the struct's 32-bit words
            q = np.ascontiguousarray(req).view(np.int32).reshape(-1, 8)
        else:
            q = np.ascontiguousarray(req).astype(np.int64).astype(np.uint32).view(np.int32).reshape(-1, 8)
        g, d = self._batch_index(group, dst, q.shape[0], "append_batch")
        out = self._batch_out(out, q.shape[0], 3, "append_batch")
        self._check(self._lib.raft_append_batch(self._h, abi.ptr(g, C.c_int64), abi.ptr(d, C.c_int32),
                                                abi.ptr(q, abi.raft_append_req), abi.ptr(out, abi.raft_append_resp),
                                                q.shape[0]), "raft_append_batch")
        return out

    def append_command_batch(self, group, replica, cmd):
        c = np.ascontiguousarray(cmd, dtype=np.uint32)
        if c.ndim != 1:
            raise ValueError(f"append_command_batch: cmd {c.shape} must be 1-D")
        g, r = self._batch_index(group, replica, c.shape[0], "append_command_batch")
        self._check(self._lib.raft_append_command_batch(self._h, abi.ptr(g, C.c_int64), abi.ptr(r, C.c_int32),
                                                        abi.ptr(c, C.c_uint32), c.shape[0]),
                    "raft_append_command_batch")


    # -- the same batches on device buffers (HBM-resident inputs) ------------
    # The engine stream does not wait for other streams: the buffers must be
    # complete before the call.  `after_stream` (a hipStream_t handle, e.g.
    # torch.cuda.current_stream().cuda_stream) orders the batch after all work
    # enqueued on that stream so far (raft_engine_wait_stream).
    def wait_stream(self, stream: int | None):
        """Order the engine stream after all work enqueued so far on `stream`
        (None / 0: the null stream)."""
        self._check(self._lib.raft_engine_wait_stream(self._h, C.c_void_p(stream or 0)), "wait_stream")

    def vote_batch_dev(self, group_ptr: int, dst_ptr: int, req_ptr: int, resp_ptr: int, n: int,
                       after_stream: int | None = None):
        """raft_vote_batch_dev: DEVICE pointers to n int64 groups, int32
        replicas, raft_vote_req and raft_vote_resp (e.g. torch tensors'
        data_ptr() on this engine's GPU)."""
        self._dev("vote_batch_dev", after_stream)
        self._check(self._lib.raft_vote_batch_dev(self._h, group_ptr, dst_ptr, req_ptr, resp_ptr, int(n)),
                    "raft_vote_batch_dev")

    def append_batch_dev(self, group_ptr: int, dst_ptr: int, req_ptr: int, resp_ptr: int, n: int,
                         after_stream: int | None = None):
        self._dev("append_batch_dev", after_stream)
        self._check(self._lib.raft_append_batch_dev(self._h, group_ptr, dst_ptr, req_ptr, resp_ptr, int(n)),
                    "raft_append_batch_dev")

    def append_command_batch_dev(self, group_ptr: int, replica_ptr: int, cmd_ptr: int, n: int,
                                 after_stream: int | None = None):
        self._dev("append_command_batch_dev", after_stream)
        self._check(self._lib.raft_append_command_batch_dev(self._h, group_ptr, replica_ptr, cmd_ptr, int(n)),
                    "raft_append_command_batch_dev")


def philox4x32_10(ctr, key):
    """The engine's Philox (host side of the shared header), for KAT checks."""
    lib = abi.load_library()
    c = (C.c_uint32 * 4)(*ctr)
    k = (C.c_uint32 * 2)(*key)
    out = (C.c_uint32 * 4)()
    lib.raft_philox4x32_10(c, k, out)
    return list(out)
