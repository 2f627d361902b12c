"""The log-tail cache read back — the Python side of include/ext/raft_debug.h,
an extension of the engine's C-ABI: a read-only window on the three words every
replica carries beside its canonical fields (t1, t2 = the terms of
log[last - 1] and log[last - 2], c1 = the command of log[last - 1]) and on the
engine's "the cache is current" flag.  RaftEngine.read_state does not export
them; the tests that hold every device-side writer of the cache to "what the
log says" (tests/test_gpu_tail_cache.py) read them here.

An extension module like its header: the entry point is declared here, once, in
`SIGNATURES`, and bound to the engine library when first used
(abi.bind_extension, as replay.py).  tests/test_tail_cache_cpu.py holds it to
the header and to the library, and tests/golden/python_api_debug.json pins this
module's surface.  There is no fallback: a library without the entry point
raises.

    from raft-kotlin_amd import debug             (importlib.import_module)
    cache, valid = debug.read_tail_cache(engine)  (n, R, 3) int32, 1 or 0
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import abi
from .engine import RaftEngine, _span

TAIL_CACHE_WORDS = ("t1", "t2", "c1")

_P = C.POINTER
SIGNATURES = {
    "raft_debug_read_tail_cache": (C.c_int, [C.c_void_p, abi.I64, abi.I64, _P(C.c_int32), _P(C.c_int32)]),
}
EXPORTED_SYMBOLS = list(SIGNATURES)


def bind(lib=None):
    """The engine library with the entry point of this extension bound
    (restype and argtypes of SIGNATURES).  Raises if the library lacks it."""
    return abi.bind_extension(lib, SIGNATURES, "_raft_debug_bound")


def read_tail_cache(engine: RaftEngine, g0: int = 0, n: int | None = None):
    """raft_debug_read_tail_cache: the words (t1, t2, c1) of every replica of
    groups [g0, g0 + n) as they are in HBM after the engine's queued work --
    an (n, R, 3) int32 array in the order of TAIL_CACHE_WORDS -- and whether
    the engine holds them to be current (1; 0: a host write left them stale
    and no consumer has rebuilt them yet).  Rebuilds nothing, writes nothing."""
    g0, n = _span("read_tail_cache", engine.G, g0, n)
    lib = bind(engine._lib)
    out = np.zeros((max(n, 0), engine.R, len(TAIL_CACHE_WORDS)), dtype=np.int32)
    valid = C.c_int32(-1)
    engine._check(lib.raft_debug_read_tail_cache(engine._h, g0, n, abi.ptr(out, C.c_int32), C.byref(valid)),
                  "raft_debug_read_tail_cache")
    return out, int(valid.value)
