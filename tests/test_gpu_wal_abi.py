"""The C-ABI of the persistence stream on a device (marker `gpu`): the struct
sizes, every refusal of include/raft_engine.h with its code, what a refused
call leaves behind, and the handle's HBM."""
import ctypes as C
import importlib

import numpy as np
import pytest

import wal_model as M
from helpers import abi

pytestmark = pytest.mark.gpu

RaftEngine = importlib.import_module("raft-kotlin_amd.engine").RaftEngine


def test_struct_sizes():
    assert C.sizeof(abi.raft_wal_cursor) == 24 and C.sizeof(abi.raft_wal_record) == 24
    assert abi.WAL_CURSOR_DTYPE.itemsize == 24 and abi.WAL_RECORD_DTYPE.itemsize == 24
    assert C.sizeof(abi.raft_wal_info) == 8 * len(abi.WAL_INFO_FIELDS)


def test_refusals_and_device_bytes():
    """RAFT_EINVAL: a null handle, info, out or buffer, a replica outside
    -1..R-1, a negative max_records, a null buffer with room, a misaligned _dev
    buffer, each bad cursor of raft_wal_write (nothing stored); RAFT_ERANGE:
    groups outside the engine; n == 0: RAFT_OK with a zeroed info.  The cursors
    count in raft_wal_device_bytes, 24 bytes a replica, and not in
    raft_engine_device_bytes; raft_engine_reset does not reach them."""
    import torch
    R, G, cap = 5, 70, 64
    with RaftEngine(abi.make_params(R=R, G=G, seed=11, log_cap=cap, cmd_ppm=500_000)) as e:
        lib = e._lib
        before = e.device_bytes
        wal = e.wal()
        assert wal.device_bytes == (24 * G * R + 255) & ~255 and e.device_bytes == before
        other = e.wal()
        assert other.device_bytes == wal.device_bytes and e.device_bytes == before
        other.close()
        e.step(40, counters=False)
        h = wal._h
        info = abi.raft_wal_info()
        rec = np.zeros(8, abi.WAL_RECORD_DTYPE)
        dev = torch.zeros(8 * 24 + 8, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        out = C.c_void_p(5)
        assert lib.raft_wal_create(e._h, None) == abi.RAFT_EINVAL
        assert lib.raft_wal_create(None, C.byref(out)) == abi.RAFT_EINVAL and b"null engine" in lib.raft_last_error()
        for fn, buf in ((lib.raft_wal_poll, rec.ctypes.data), (lib.raft_wal_poll_dev, dev.data_ptr())):
            assert fn(None, 0, G, -1, buf, 8, C.byref(info)) == abi.RAFT_EINVAL
            assert fn(h, 0, G, -1, buf, 8, None) == abi.RAFT_EINVAL
            for replica in (R, -2):
                assert fn(h, 0, G, replica, buf, 8, C.byref(info)) == abi.RAFT_EINVAL
                assert b"replica" in lib.raft_last_error()
            assert fn(h, 0, G, -1, buf, -1, C.byref(info)) == abi.RAFT_EINVAL
            assert b"max_records must be >= 0" in lib.raft_last_error()
            assert fn(h, 0, G, -1, None, 8, C.byref(info)) == abi.RAFT_EINVAL
            assert b"null record buffer with max_records > 0" in lib.raft_last_error()
            for g0, n in ((G, 1), (-1, 2), (G - 1, 2), (0, -1)):
                info.delivered = info.pending = 5
                assert fn(h, g0, n, -1, buf, 8, C.byref(info)) == abi.RAFT_ERANGE
                assert info.delivered == 0 and info.pending == 0
            info.pending = info.lost = 5
            assert fn(h, 3, 0, -1, buf, 8, C.byref(info)) == abi.RAFT_OK and info.pending == 0 and info.lost == 0
        assert lib.raft_wal_poll_dev(h, 0, G, -1, dev.data_ptr() + 4, 8, C.byref(info)) == abi.RAFT_EINVAL
        assert b"8-byte aligned" in lib.raft_last_error()
        assert lib.raft_wal_poll(h, 0, G, -1, rec.ctypes.data + 4, 1, C.byref(info)) == abi.RAFT_OK   # a host buffer may lie anywhere
        cur = wal.cursors()                                               # the refused calls stored nothing: only that one
        assert cur["term"][0, 0] > 0 and cur["stable"][0, 0] == 0         # record, replica (0, 0)'s HARDSTATE, moved a cursor
        assert np.array_equal(cur.reshape(-1)[1:], M.fresh(G, R).reshape(-1)[1:])
        assert lib.raft_wal_read(h, 0, 1, None) == abi.RAFT_EINVAL and lib.raft_wal_write(h, 0, 1, None) == abi.RAFT_EINVAL
        assert lib.raft_wal_read(h, G, 1, cur.ctypes.data) == abi.RAFT_ERANGE
        assert lib.raft_wal_write(h, G - 1, 2, cur.ctypes.data) == abi.RAFT_ERANGE
        assert lib.raft_wal_read(h, 0, 0, None) == abi.RAFT_OK and lib.raft_wal_write(h, G, 0, None) == abi.RAFT_OK
        wal.poll()
        good = wal.cursors()
        for field, v, word in (("stable", -1, b"stable"), ("stable", cap + 1, b"stable"), ("floor", -1, b"floor"),
                               ("vote", R + 1, b"vote"), ("vote", -2, b"vote"), ("term", -1, b"term"), ("pad", 7, b"pad")):
            bad = good.copy()
            bad[field][G - 1, R - 1] = v
            assert lib.raft_wal_write(h, 0, G, bad.ctypes.data) == abi.RAFT_EINVAL, field
            assert word in lib.raft_last_error()
            assert np.array_equal(wal.cursors(), good), field
        bad = good.copy()
        bad["floor"][0, 0] = bad["stable"][0, 0] + 1
        assert lib.raft_wal_write(h, 0, G, bad.ctypes.data) == abi.RAFT_EINVAL and np.array_equal(wal.cursors(), good)
        edge = good.copy()                                                # the ends of every range are accepted
        edge[0, 0] = (0, -1, cap, 0, cap, 0)
        edge[0, 1] = (2 ** 31 - 1, R, 0, -5, 0, 0)                       # votedFor is a node id: replica index + 1
        assert lib.raft_wal_write(h, 0, G, edge.ctypes.data) == abi.RAFT_OK and np.array_equal(wal.cursors(), edge)
        wal.set_cursors(good)
        e.reset()
        assert np.array_equal(wal.cursors(), good)                        # raft_engine_reset does not reach the handle
        assert lib.raft_wal_reset(h) == abi.RAFT_OK and np.array_equal(wal.cursors(), M.fresh(G, R))
        assert lib.raft_wal_reset(None) == abi.RAFT_EINVAL and lib.raft_wal_device_bytes(None) == 0
        assert lib.raft_wal_destroy(None) == abi.RAFT_OK
