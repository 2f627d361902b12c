"""Leadership transfer on the GPU (marker `gpu`): raft_transfer_batch*,
raft_engine_resolve_transfers* and raft_engine_evacuate* against the oracle
driven through tests/transfer_model.py (read_state -> model -> write_state).
Every comparison is exact."""
import ctypes as C
import importlib

import numpy as np
import pytest

import transfer_model as TM
from helpers import abi, high_g0

pytestmark = pytest.mark.gpu

eng_mod = importlib.import_module("raft-kotlin_amd.engine")
service = importlib.import_module("raft-kotlin_amd.service")
RaftEngine = eng_mod.RaftEngine
RaftError = eng_mod.RaftError


def same(got, want, label=""):
    assert got.dtype == want.dtype and len(got) == len(want), (label, got.dtype, len(got), len(want))
    if not np.array_equal(got, want):
        at = int(np.nonzero(got != want)[0][0])
        raise AssertionError(f"{label}: {int((got != want).sum())} records differ; first at {at}: {got[at]} vs {want[at]}")


@pytest.mark.parametrize("R,G,variant", TM.PARITY_CASES, ids=[f"R{c[0]}-G{c[1]}-{c[2]}" for c in TM.PARITY_CASES])
def test_parity_with_the_oracle(R, G, variant):
    """40 steps, a transfer batch over [3, G - 2) with seeded targets and 7
    duplicate groups, 3 steps, resolve, an evacuate of replicas 0 and 2, 40
    steps: tickets, states, info, state, logs, digest and counter rows equal
    the oracle's under the model, bit for bit."""
    want, _ = TM.host_parity_run(R, G, variant)
    with RaftEngine(abi.make_params(**TM.RM.parity_kw(R, G, variant))) as e:
        got = TM.parity_run(e, f"R{R} G{G} {variant}")
    TM.assert_same_points(got, want, R)


def test_parity_at_the_top_of_the_global_ids():
    """One shard whose last group has global id 2^32 - 1: the calls index by
    the engine-local group, the steps after them draw by the global id."""
    g0 = high_g0(203)["top"]
    want, _ = TM.host_parity_run(5, 203, "flat", g0)
    with RaftEngine(abi.make_params(g0=g0, **TM.RM.parity_kw(5, 203, "flat"))) as e:
        got = TM.parity_run(e, "R5 G203 flat top")
    TM.assert_same_points(got, want, 5)


def test_host_and_device_buffers_agree():
    """The host forms and the _dev forms on two engines in the same state give
    identical tickets, states, info and digests, and the _dev forms write
    nothing beyond their records."""
    import torch
    R, G = 5, 203
    kw = TM.RM.parity_kw(R, G, "flat")
    groups, targets = TM.parity_messages(R, G)
    n = len(groups)
    mask = np.full(G - 5, TM.EVACUATE_MASK, np.uint8)
    with RaftEngine(abi.make_params(**kw)) as a, RaftEngine(abi.make_params(**kw)) as b:
        for e in (a, b):
            e.step(40, counters=False)
        tk = a.transfer(groups, targets)
        dg = torch.from_numpy(groups).to("cuda:0")
        dt = torch.from_numpy(targets).to("cuda:0")
        dk = torch.full(((n + 1) * 4,), -7, dtype=torch.int32, device="cuda:0")
        ds = torch.full(((n + 1) * 4,), -7, dtype=torch.int32, device="cuda:0")
        dm = torch.from_numpy(mask).to("cuda:0")
        torch.cuda.synchronize()
        assert b.transfer_dev(dg.data_ptr(), dt.data_ptr(), dk.data_ptr(), n) == abi.RAFT_OK
        raw = dk.cpu().numpy()
        same(raw[:-4].view(abi.TRANSFER_TICKET_DTYPE), tk, "device tickets")
        assert (raw[-4:] == -7).all() and (tk["status"] == TM.SENT).sum() > 0
        assert a.digest() == b.digest()
        for e in (a, b):
            e.step(3, counters=False)
        st = a.resolve_transfers(groups, tk)
        assert b.resolve_transfers_dev(dg.data_ptr(), dk.data_ptr(), ds.data_ptr(), n) == abi.RAFT_OK
        raw = ds.cpu().numpy()
        same(raw[:-4].view(abi.TRANSFER_STATE_DTYPE), st, "device states")
        assert (raw[-4:] == -7).all() and (st["status"] == TM.COMPLETED).sum() > 0
        info = a.evacuate(mask, g0=3)
        assert b.evacuate_dev(dm.data_ptr(), len(mask), g0=3) == info and info["sent"] > 0
        assert a.digest() == b.digest()


def test_error_paths():
    """A group at G fails the batch with RAFT_ERANGE and nothing is written;
    n == 0 is RAFT_OK; null pointers are RAFT_EINVAL; a resolve fills every
    record whatever it returns."""
    R, G = 5, 70
    with RaftEngine(abi.make_params(R=R, G=G, seed=11, log_cap=64, cmd_ppm=100_000)) as e:
        e.step(40, counters=False)
        before = e.digest()
        groups = np.arange(G + 1, dtype=np.int64)
        with pytest.raises(RaftError, match="outside the engine"):
            e.transfer(groups)
        with pytest.raises(RaftError, match="outside the engine"):
            e.transfer([5, -1], [0, 0])
        assert e.digest() == before
        for g0, n in ((G, 1), (-1, 2), (G - 1, 2)):
            with pytest.raises(RaftError, match="outside the engine"):
                e.evacuate(np.full(n, 0xFF, np.uint8), g0=g0)
        assert e.digest() == before
        lib, h = e._lib, e._h
        buf = np.zeros(64, np.int64)
        p = C.c_void_p(buf.ctypes.data)
        info = abi.raft_evacuate_info()
        info.led = 5
        assert lib.raft_transfer_batch(h, None, None, None, 0) == abi.RAFT_OK
        assert lib.raft_engine_resolve_transfers(h, None, None, None, 0) == abi.RAFT_OK
        assert lib.raft_engine_evacuate(h, G, 0, None, C.byref(info)) == abi.RAFT_OK and info.led == 0
        assert len(e.transfer([])) == 0 and len(e.resolve_transfers([], np.zeros(0, abi.TRANSFER_TICKET_DTYPE))) == 0
        assert e.evacuate(np.zeros(0, np.uint8)) == dict.fromkeys(abi.EVACUATE_INFO_FIELDS, 0)
        for args in ((None, p, p), (p, None, p), (p, p, None)):
            for fn in (lib.raft_transfer_batch, lib.raft_transfer_batch_dev, lib.raft_engine_resolve_transfers,
                       lib.raft_engine_resolve_transfers_dev):
                assert fn(h, *args, 1) == abi.RAFT_EINVAL
        assert lib.raft_transfer_batch(h, p, p, p, -1) == abi.RAFT_EINVAL
        assert lib.raft_engine_evacuate(h, 0, 4, None, C.byref(info)) == abi.RAFT_EINVAL
        assert lib.raft_engine_evacuate(h, 0, 4, p, None) == abi.RAFT_EINVAL
        assert lib.raft_engine_evacuate_dev(h, 0, 4, None, C.byref(info)) == abi.RAFT_EINVAL
        assert e.digest() == before
        # an INVALID target reads and writes nothing; resolve: a group outside, then a SENT ticket with a bad target
        tk = e.transfer([3, 4], [R, -2])
        assert tk.tolist() == [(-1, 0, -1, TM.INVALID)] * 2 and e.digest() == before
        tickets = np.array([(0, 1, 1, TM.SENT), (0, 1, R, TM.SENT), (0, 1, 1, TM.BUSY)], dtype=abi.TRANSFER_TICKET_DTYPE)
        want, rc = TM.resolve(e.read_state(), [G, 0, 0], tickets, R)
        same(e.resolve_transfers([G, 0, 0], tickets, check=False), want, "records of a refused resolve")
        assert e.last_status == rc == abi.RAFT_ERANGE
        want, rc = TM.resolve(e.read_state(), [0, 0, 0], tickets, R)
        same(e.resolve_transfers([0, 0, 0], tickets, check=False), want, "records of a bad ticket")
        assert e.last_status == rc == abi.RAFT_EINVAL
        with pytest.raises(RaftError):
            e.resolve_transfers([0, 0, 0], tickets)
        assert e.digest() == before


def test_crafted_statuses_on_the_device():
    """The crafted groups of transfer_model.crafted() written into an engine (the
    last terms through write_log, so the tail cache is rebuilt first): the
    tickets and the one changed word per SENT ticket equal the model's."""
    w, lt, tgt, want, names = TM.crafted()
    R, G, cap = 5, len(names), 8
    terms = np.zeros((G, R, cap), np.int32)
    terms[:, :, :5] = 1
    for r in range(R):
        last = w[:, r * abi.NUM_FIELDS + abi.F_INDEX["last"]]
        terms[np.arange(G), r, last - 1] = lt[:, r]
    with RaftEngine(abi.make_params(R=R, G=G, log_cap=cap, mode=1)) as e:
        e.write_state(w)
        e.write_log(terms, np.zeros((G, R, cap), np.uint32))
        base = e.read_state()
        model = w.copy()
        want_tk, _ = TM.transfer(model, np.arange(G), tgt, R, lt)
        same(want_tk, want, "the model on the crafted groups")
        same(e.transfer(np.arange(G), tgt), want, "crafted tickets")
        after = e.read_state()
        assert np.array_equal(np.argwhere(after != base), np.argwhere(model != w)) and (after[after != base] == 1).all()
        e.write_state(w)
        mask = np.full(G, 0b00010, np.uint8)                       # the leader of every group but one
        model = w.copy()
        assert e.evacuate(mask) == TM.evacuate(model, mask, R, 0, lt)
        after = e.read_state()
        assert np.array_equal(np.argwhere(after != base), np.argwhere(model != w)) and (after[after != base] == 1).all()


def test_drain_node_matches_the_host():
    """RaftService.drain_node on the engine takes the turns and leaves the
    groups the same call over the oracle Host does, and the restart's downtime
    then costs no group its leader."""
    h = TM.Host(**TM.DRAIN_KW)
    want = TM.drain_scenario(h, service.RaftService, drain=True)
    h.close()
    with RaftEngine(abi.make_params(**TM.DRAIN_KW)) as e:
        got = TM.drain_scenario(e, service.RaftService, drain=True)
    assert got == want and got["remaining"] == 0 and min(got["during"]) >= got["before"], (got, want)
