"""WAL replay — the Python side of include/ext/raft_replay.h, an extension of
the engine's C-ABI: the inverse of RaftWal.poll.  A batch of persistence-stream
records is applied to the replicas it names, on the device, between two step
launches.

An extension module like its header: the record and the two entry points are
declared here, once, with `abi.record` and in `SIGNATURES`, and bound to the
engine library when first used.  tests/test_replay_abi_cpu.py holds them to the
header and to the library, and tests/golden/python_api_replay.json pins this
module's surface.  There is no fallback: a library without the entry points
raises.

    from raft-kotlin_amd import replay            (importlib.import_module)
    replay.replay(engine, records)                host records
    replay.replay_dev(engine, ptr, n)             records in DEVICE memory
    replay.image_records(image, g, r)             a WalImage's records of one replica
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import abi
from .engine import RaftEngine, RaftError, WalImage

# the info (64 bytes) and the flag of raft_wal_replay*
raft_replay_info = abi.record("raft_replay_info", ("applied replicas hardstates truncates entries malformed reserved[2]",
                                                   abi.I64))
REPLAY_KEEP_VOLATILE = 1
REPLAY_INFO_FIELDS = raft_replay_info.scalars

_P = C.POINTER
SIGNATURES = {
    "raft_wal_replay": (C.c_int, [C.c_void_p, C.c_void_p, abi.I64, abi.U32, _P(raft_replay_info)]),
    "raft_wal_replay_dev": (C.c_int, [C.c_void_p, C.c_void_p, abi.I64, abi.U32, _P(raft_replay_info)]),
}
EXPORTED_SYMBOLS = list(SIGNATURES)


def bind(lib=None):
    """The engine library with the entry points of this extension bound
    (restype and argtypes of SIGNATURES).  Raises if the library lacks one."""
    return abi.bind_extension(lib, SIGNATURES, "_raft_replay_bound")


def _call(engine: RaftEngine, name: str, ptr: int, n: int, keep_volatile: bool) -> dict:
    """One raft_wal_replay* call.  A refused batch (RAFT_EINVAL with malformed
    records counted) raises RaftError; the exception's `info` holds the info
    dict, malformed included."""
    lib = bind(engine._lib)
    ri = raft_replay_info()
    rc = getattr(lib, name)(engine._h, C.c_void_p(ptr or 0), n, REPLAY_KEEP_VOLATILE if keep_volatile else 0, C.byref(ri))
    try:
        engine._check(rc, name)
    except RaftError as err:
        err.info = abi.info_dict(ri)
        raise
    return abi.info_dict(ri)


def replay(engine: RaftEngine, records, *, keep_volatile: bool = False) -> dict:
    """raft_wal_replay: apply a batch of persistence-stream records
    (abi.WAL_RECORD_DTYPE: what RaftWal.poll of this or a like engine returned,
    whole or in the pieces max_records cut, or image_records) to the replicas
    they name, on the device.  A touched replica gets the hard state of its
    HARDSTATE, lastIndex = physLen from its last record, its ENTRYs stored, and
    the volatile state of a restart (FOLLOWER, commitIndex 0, a fresh election
    timeout, no sessions); with keep_volatile=True role, commitIndex, timers
    and sessions stay (a standby that is never stepped).  One malformed record
    refuses the whole batch before anything is written: RaftError, its
    `info["malformed"]` says how many.  Returns applied, replicas, hardstates,
    truncates, entries, malformed (raft_replay_info)."""
    rec = np.asarray(records)
    if rec.ndim != 1 or rec.dtype != abi.WAL_RECORD_DTYPE:
        raise ValueError(f"replay: records {rec.shape} {rec.dtype} must be a 1-D array of abi.WAL_RECORD_DTYPE")
    rec = np.ascontiguousarray(rec)
    return _call(engine, "raft_wal_replay", rec.ctypes.data if len(rec) else 0, len(rec), keep_volatile)


def replay_dev(engine: RaftEngine, ptr: int, n: int, *, keep_volatile: bool = False,
               after_stream: int | None = None) -> dict:
    """replay with the n records in DEVICE memory (24 bytes each, 8-byte
    aligned, e.g. the buffer RaftWal.poll_dev of another engine filled);
    returns once the kernels finished."""
    if not isinstance(n, (int, np.integer)) or isinstance(n, bool) or not 0 <= n <= 0x7FFFFFFF:
        raise ValueError(f"replay_dev: n must be an integer in 0..{0x7FFFFFFF}, not {n!r}")
    if n > 0 and not ptr:
        raise ValueError("replay_dev: a device buffer is required")
    if (ptr or 0) % 8:
        raise ValueError("replay_dev: the record buffer must be 8-byte aligned")
    if after_stream is not None:
        engine.wait_stream(after_stream)
    n = int(n)
    return _call(engine, "raft_wal_replay_dev", ptr, n, keep_volatile)


def image_records(image: WalImage, g: int, r: int) -> np.ndarray:
    """The records that rebuild replica r of group g from a WalImage
    (abi.WAL_RECORD_DTYPE, a batch of replay): its HARDSTATE, a TRUNCATE(0),
    then one ENTRY per persisted entry, ascending.  Of a ring image only the
    newest log_window entries can be replayed in one batch: cut the ENTRYs to
    them (and drop the TRUNCATE) before replaying."""
    if not (0 <= g < image.G and 0 <= r < image.R):
        raise IndexError((g, r))
    n = int(image.length[g, r])
    rec = np.zeros(n + 2, dtype=abi.WAL_RECORD_DTYPE)
    rec["group"], rec["replica"] = g, r
    rec[0] = (g, r, abi.WAL_HARDSTATE, -1, int(image.term[g, r]), 0, int(image.vote[g, r]))
    rec[1] = (g, r, abi.WAL_TRUNCATE, 0, 0, 0, 0)
    rec["kind"][2:] = abi.WAL_ENTRY
    rec["index"][2:] = np.arange(n)
    rec["term"][2:], rec["cmd"][2:] = image.terms[g, r, :n], image.cmds[g, r, :n]
    return rec
