"""The proposal outbox on the GPU (marker `gpu`): raft_engine_outbox_configure,
raft_outbox_submit*, raft_engine_outbox_pump*, raft_engine_outbox_read / write
against the oracle driven through tests/outbox_model.py.  Every comparison is
exact."""
import ctypes as C
import importlib

import numpy as np
import pytest

import outbox_model as OM
from helpers import abi

pytestmark = pytest.mark.gpu

eng_mod = importlib.import_module("raft-kotlin_amd.engine")
service = importlib.import_module("raft-kotlin_amd.service")
RaftEngine = eng_mod.RaftEngine
RaftError = eng_mod.RaftError

# raft_build_kernel_source_id() of the commit this feature was built on
PARENT_KERNEL_SOURCE_ID = "1866b1ae2e1d"


def same(got, want, label=""):
    assert got.dtype == want.dtype and len(got) == len(want), (label, got.dtype, len(got), len(want))
    if not np.array_equal(got, want):
        at = int(np.flatnonzero(got != want)[0])
        raise AssertionError(f"{label}: {int((got != want).sum())} records differ; first at {at}: {got[at]} vs {want[at]}")


def crafted_engine(textbook: bool) -> RaftEngine:
    e = RaftEngine(abi.make_params(R=OM.CR, G=OM.CG, log_cap=OM.CCAP, **(dict(mode=abi.MODE_TEXTBOOK) if textbook else {})))
    OM.load_crafted(e)
    return e


@pytest.mark.parametrize("textbook", [False, True], ids=["reference", "textbook"])
def test_crafted_groups_host_form(textbook):
    """One group per verdict (outbox_model.crafted): done, queue and info are
    the records written out by hand, record for record, and the state is the
    oracle's under the model."""
    h = OM.crafted_host(textbook)
    h.outbox_pump()
    with crafted_engine(textbook) as e:
        same(e.outbox_read(), OM.CRAFTED_QUEUE, "written queue")
        info, done = e.outbox_pump()
        assert info == OM.CRAFTED_INFO and e.last_status == abi.RAFT_OK, info
        same(done, OM.CRAFTED_DONE, "done")
        same(e.outbox_read(), OM.CRAFTED_LEFT, "queue")
        assert np.array_equal(e.read_state(), h.read_state()) and e.digest() == h.digest()
        want2, wdone2 = h.outbox_pump()
        info2, done2 = e.outbox_pump()
        assert info2 == want2 and len(done2) == len(wdone2) == 0
        same(e.outbox_read(), h.outbox_read(), "queue after a second pump")
    h.close()


@pytest.mark.parametrize("max_done", [0, 1, 2, 3])
def test_crafted_groups_device_form_and_the_cut(max_done):
    """raft_engine_outbox_pump_dev into a device buffer, cut at 0, at 1, in the
    middle and at the end of the three done records: the records and nothing
    beyond them; the rest stays, in order, for the next pump."""
    import torch
    want_done, want_left, want_info = OM.crafted_cut(max_done) if max_done < 3 else \
        (OM.CRAFTED_DONE, OM.CRAFTED_LEFT, OM.CRAFTED_INFO)
    with crafted_engine(True) as e:
        buf = torch.full(((max_done + 1) * 8,), -7, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        info, n = e.outbox_pump_dev(buf.data_ptr(), max_done)
        raw = buf.cpu().numpy()
        assert info == want_info and n == len(want_done), (info, n)
        same(raw[: 8 * n].view(abi.OUTBOX_DONE_DTYPE), want_done, "device done")
        assert (raw[8 * n:] == -7).all()
        same(e.outbox_read(), want_left, "queue")
        info2, rest = e.outbox_pump()
        same(np.concatenate([want_done, rest]), OM.CRAFTED_DONE, "both pumps")
        with pytest.raises(ValueError, match="16-byte"):
            e.outbox_pump_dev(buf.data_ptr() + 8, 1)


def test_below_a_window_is_unknown():
    w, t, c = OM.crafted_ring()
    with RaftEngine(abi.make_params(**OM.RING_KW)) as e:
        e.write_state(w)
        e.write_log(t, c)
        e.outbox_configure(8)
        e.outbox_write(OM.RING_QUEUE)
        info, done = e.outbox_pump()
        assert info == OM.RING_INFO and e.last_status == abi.RAFT_EWINDOW and len(done) == 0
        same(e.outbox_read(), OM.RING_QUEUE, "queue")


def test_submit_forms_agree():
    """raft_outbox_submit and raft_outbox_submit_dev append the same records,
    at the tail, in batch order; a refused _dev batch leaves the queue alone."""
    import torch
    kw = OM.parity_kw(5, "textbook", "flat")
    rng = np.random.default_rng(3)
    with RaftEngine(abi.make_params(**kw)) as a, RaftEngine(abi.make_params(**kw)) as d:
        for e in (a, d):
            e.step(7, counters=False)
            e.outbox_configure(2048)
        for k, size in enumerate((1, 300, 700)):
            groups, cmds, tags = OM.batch_of(rng, size, a.G, k)
            a.outbox_submit(groups, cmds, tags)
            tg, tc, tt = (torch.from_numpy(x.view(np.int64) if x.dtype == np.int64 else x.view(np.int32)).to("cuda:0")
                          for x in (groups, cmds, tags))
            torch.cuda.synchronize()
            d.outbox_submit_dev(tg.data_ptr(), tc.data_ptr(), tt.data_ptr(), size)
        q = a.outbox_read()
        same(d.outbox_read(), q, "device submit")
        assert len(q) == 1001 and (q["born"] == 7).all() and (q["status"] == OM.NEW).all()
        bad = torch.tensor([1, a.G], dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        with pytest.raises(RaftError, match="outside the engine"):
            d.outbox_submit_dev(bad.data_ptr(), tc.data_ptr(), tt.data_ptr(), 2)
        same(d.outbox_read(), q, "after a refused device submit")


@pytest.mark.parametrize("R,mode,log", OM.PARITY_CASES, ids=[f"R{c[0]}-{c[1]}-{c[2]}" for c in OM.PARITY_CASES])
def test_parity_with_the_oracle(R, mode, log):
    """outbox_model.parity_run on the engine: after every pump the queue, the
    done stream, the info, the return code, the state, the logs and the digest
    equal the oracle Host's, and so do the counter rows of the steps in between
    (a ring: up to the oracle's first window miss)."""
    want = OM.host_parity_run(R, mode, log)
    with RaftEngine(abi.make_params(**OM.parity_kw(R, mode, log))) as e:
        got = OM.parity_run(e, f"R{R} {mode} {log}")
    OM.assert_same_points(got, want, R)


@pytest.mark.parametrize("mode", ["reference", "textbook"])
def test_an_engine_without_an_outbox_is_unchanged(mode):
    """The same steps and restarts on an engine that never configures an
    outbox: its counter rows and digests equal the outbox engine's up to the
    first pump that proposes something (from then on the logs differ by the
    proposals)."""
    want = OM.host_parity_run(5, mode, "flat")
    first = OM.first_retry(want)
    with RaftEngine(abi.make_params(**OM.parity_kw(5, mode, "flat"))) as e:
        plain = OM.parity_run(e, outbox=False)
    before = [p for p in want[:first] if "counters" in p]
    assert len(before) >= 2
    for a, b in zip(plain, before):
        assert np.array_equal(a["counters"], b["counters"]) and a["digest"] == b["digest"], b["what"]


def scrambled(x, L: int):
    """L records (and L // 2 more, still NEW) over 203 groups in every state a
    pump meets, interleaved: submit, pump, steps, a restart, a second submit,
    then the queue read, permuted and written back."""
    rng = np.random.default_rng(100 + L)
    x.step(30)
    x.outbox_configure(8192, 25)
    if L:
        x.outbox_submit(np.arange(L, dtype=np.int64) * 7 % x.G, (5_000_000 + np.arange(L)).astype(np.uint32),
                        np.arange(L, dtype=np.int64))
    first = x.outbox_pump()
    x.step(6)
    x.restart(ppm=200_000)
    x.step(4)
    if L // 2:
        x.outbox_submit(rng.integers(0, x.G, L // 2), (6_000_000 + np.arange(L // 2)).astype(np.uint32),
                        10_000 + np.arange(L // 2, dtype=np.int64))
    q = x.outbox_read()
    x.outbox_write(q[rng.permutation(len(q))])
    return first


@pytest.mark.parametrize("L", [0, 1, 63, 64, 65, 700, 5000])
def test_queue_lengths_where_the_split_can_go_wrong(L):
    """Queue lengths around a wave, and 5,000 + 2,500 records over 203 groups:
    past a split workgroup's 256 records and the verdict pass's 32, runs of one
    group across those boundaries, done, retried and kept records interleaved.
    Two pumps (the first cut in the middle of its done records) equal the
    model's, record for record."""
    kw = OM.parity_kw(5, "textbook", "flat")
    h = OM.Host(**kw)
    with RaftEngine(abi.make_params(**kw)) as e:
        for x in (h, e):
            x.first = scrambled(x, L)
        assert e.first[0] == h.first[0]
        same(e.first[1], h.first[1], "first done")
        same(e.outbox_read(), h.outbox_read(), "scrambled queue")
        n_fin = sum(h.outbox_pump(0)[0][k] for k in ("deferred",))
        assert e.outbox_pump(0)[0]["deferred"] == n_fin
        for max_done in (n_fin // 2, None):
            want_info, want_done = h.outbox_pump(max_done)
            info, done = e.outbox_pump(max_done)
            assert info == want_info, (max_done, info, want_info)
            same(done, want_done, f"done (max_done {max_done})")
            same(e.outbox_read(), h.outbox_read(), f"queue (max_done {max_done})")
            assert e.digest() == h.digest()
            for x in (h, e):
                x.step(3)
        if L >= 700:
            assert want_info["committed"] and want_info["retried"] and want_info["pending"], want_info
    h.close()


def test_resume_on_a_second_engine():
    """outbox_write of a read queue on a second engine in the same state, then
    identical pumps on both."""
    kw = OM.parity_kw(5, "textbook", "flat")
    with RaftEngine(abi.make_params(**kw)) as a, RaftEngine(abi.make_params(**kw)) as b:
        scrambled(a, 700)
        b.write_state(a.read_state())
        b.write_log(*a.read_log())
        b.step_index = a.step_index
        b.outbox_configure(1050, 25)
        b.outbox_write(a.outbox_read())
        assert a.digest() == b.digest()
        for _ in range(3):
            ia, da = a.outbox_pump()
            ib, db = b.outbox_pump()
            assert ia == ib and a.last_status == b.last_status
            same(db, da, "done")
            same(b.outbox_read(), a.outbox_read(), "queue")
            assert np.array_equal(a.step(5), b.step(5)) and a.digest() == b.digest()
        assert ia["queued"] > 0


def test_bytes_configure_reset_and_refusals():
    """device_bytes grows at configure and not before; trim_staging keeps the
    queue; reset empties it; the refusals of the header, with nothing stored."""
    R, G = 3, 8
    with RaftEngine(abi.make_params(R=R, G=G, log_cap=16)) as e:
        lib, h = e._lib, e._h
        e.step(3, counters=False)
        b0 = e.device_bytes
        n, info = C.c_int64(5), abi.raft_outbox_info()
        one = np.zeros(1, np.int64)
        p = C.c_void_p(one.ctypes.data)
        for rc in (lib.raft_outbox_submit(h, p, p, p, 1), lib.raft_engine_outbox_pump(h, None, 0, C.byref(n), C.byref(info)),
                   lib.raft_engine_outbox_read(h, None, 0, C.byref(n)), lib.raft_engine_outbox_write(h, None, 0)):
            assert rc == abi.RAFT_EINVAL and b"not configured" in lib.raft_last_error()
        for cap, exp in ((0, 0), (-1, 0), (4, -1), (2 ** 31, 0)):
            assert lib.raft_engine_outbox_configure(h, cap, exp) == abi.RAFT_EINVAL
        assert e.device_bytes == b0
        e.outbox_configure(4)
        assert e.device_bytes >= b0 + 2 * 4 * 48
        e.outbox_submit([1, 2], [11, 12], [101, 102])
        before = e.outbox_read()
        for groups, code in (([1, 2, 3], abi.RAFT_EFULL), ([1, G], abi.RAFT_ERANGE), ([-1], abi.RAFT_ERANGE)):
            g = np.array(groups, np.int64)
            c = np.zeros(len(g), np.uint32)
            assert lib.raft_outbox_submit(h, C.c_void_p(g.ctypes.data), C.c_void_p(c.ctypes.data),
                                          C.c_void_p(g.ctypes.data), len(g)) == code
            same(e.outbox_read(), before, "after a refused submit")
        assert lib.raft_outbox_submit(h, None, None, None, 0) == abi.RAFT_OK
        assert lib.raft_engine_outbox_configure(h, 8, 0) == abi.RAFT_EINVAL and b"not empty" in lib.raft_last_error()
        bad = before.copy()
        for field, value, code in (("group", G, abi.RAFT_ERANGE), ("status", 7, abi.RAFT_EINVAL),
                                   ("tries", -1, abi.RAFT_EINVAL), ("pad", 1, abi.RAFT_EINVAL)):
            bad[:] = before
            bad[field][1] = value
            assert lib.raft_engine_outbox_write(h, C.c_void_p(bad.ctypes.data), 2) == code
        bad[:] = before
        bad["status"][0], bad["replica"][0], bad["index"][0] = 0, R, 2
        assert lib.raft_engine_outbox_write(h, C.c_void_p(bad.ctypes.data), 2) == abi.RAFT_EINVAL
        bad["replica"][0], bad["index"][0] = 0, 16
        assert lib.raft_engine_outbox_write(h, C.c_void_p(bad.ctypes.data), 2) == abi.RAFT_EINVAL
        five = np.zeros(5, abi.OUTBOX_ENTRY_DTYPE)
        assert lib.raft_engine_outbox_write(h, C.c_void_p(five.ctypes.data), 5) == abi.RAFT_EFULL
        same(e.outbox_read(), before, "after refused writes")
        assert lib.raft_engine_outbox_pump(h, None, 1, C.byref(n), C.byref(info)) == abi.RAFT_EINVAL
        assert lib.raft_engine_outbox_pump(h, None, -1, C.byref(n), C.byref(info)) == abi.RAFT_EINVAL
        assert lib.raft_engine_outbox_pump(h, None, 0, None, C.byref(info)) == abi.RAFT_EINVAL
        assert lib.raft_engine_outbox_read(h, C.c_void_p(five.ctypes.data), 1, C.byref(n)) == abi.RAFT_EINVAL and n.value == 2
        same(e.outbox_read(), before, "after refused pumps")
        e.outbox_pump()
        e.trim_staging()
        assert e.device_bytes >= b0 + 2 * 4 * 48 and e.outbox_len() == 2
        e.reset()
        assert e.outbox_len() == 0 and e.step_index == 0
        e.outbox_configure(8, 5)


def test_the_service_submits_reliably():
    """RaftService.submit_reliable / completions / pump_until_idle end to end on
    8 groups with string commands: every command completes COMMITTED exactly
    once and stands once in its leader's log."""
    kw = dict(OM.NM.LIVE_KW, G=8)
    with RaftEngine(abi.make_params(**kw)) as e:
        e.outbox_configure(64)
        svc = service.RaftService(e)
        e.step(20, counters=False)
        groups = [g for g in range(8) for _ in range(3)]
        names = [f"set k{g}={j}" for g in range(8) for j in range(3)]
        tags = svc.submit_reliable(groups, names)
        assert tags.tolist() == list(range(24)) and e.outbox_len() == 24
        done = svc.pump_until_idle(60)
        assert e.outbox_len() == 0 and sorted(d[0] for d in done) == list(range(24))
        assert {d[1] for d in done} == set(names) and all(d[2] == "COMMITTED" and d[5] >= 1 for d in done)
        for tag, name, _status, index, term, _tries, _age in done:
            entries = svc.leader(groups[tag]).entries()
            assert entries[index] == f"{term}: {name}" and sum(x.endswith(": " + name) for x in entries) == 1
        assert svc.submit_reliable([0], ["again"]).tolist() == [24]


def test_the_outbox_and_the_leader_watch_share_an_allocation():
    """The queue lives behind the watch's seen pairs.  A watch in use before
    configure keeps what it reported; one first used afterwards starts from
    "nothing reported"; both orders then poll the same events and pump the same
    records, and reset empties both."""
    kw = OM.parity_kw(5, "textbook", "flat")
    groups = np.arange(100, dtype=np.int64) * 2
    cmds = (7_000_000 + np.arange(100)).astype(np.uint32)
    with RaftEngine(abi.make_params(**kw)) as a, RaftEngine(abi.make_params(**kw)) as b:
        for e in (a, b):
            e.step(40, counters=False)
        first_a = a.poll_leaders()
        a.outbox_configure(256)
        b.outbox_configure(256)
        first_b = b.poll_leaders()
        assert first_a[0] == first_b[0] and first_a[0]["delivered"] > 0
        same(first_b[1], first_a[1], "first poll")
        assert np.array_equal(a.read_watch(), b.read_watch())
        assert a.poll_leaders()[0]["delivered"] == 0                # configure kept what the watch had reported
        for e in (a, b):
            e.outbox_submit(groups, cmds, groups)
            e.pumped = e.outbox_pump()
            e.step(10, counters=False)
        with pytest.raises(RaftError, match="not empty"):
            a.outbox_configure(512)
        pa, pb = a.poll_leaders(), b.poll_leaders()
        assert pa[0] == pb[0] and pa[0]["delivered"] > 0
        same(pb[1], pa[1], "second poll")
        ia, da = a.outbox_pump()
        ib, db = b.outbox_pump()
        assert ia == ib == dict(ia, queued=100) and a.pumped[0] == b.pumped[0] and ia["committed"] > 0
        same(db, da, "done")
        same(b.outbox_read(), a.outbox_read(), "queue")
        assert np.array_equal(a.read_watch(), b.read_watch()) and a.digest() == b.digest()
        a.reset()
        assert a.outbox_len() == 0 and (a.read_watch() == np.array(abi.WATCH_UNSEEN)).all()
        a.outbox_configure(512, 3)                                  # empty: a larger queue, the pairs move over
        a.step(40, counters=False)
        again = a.poll_leaders()
        assert again[0] == first_a[0]
        same(again[1], first_a[1], "the first poll after a reset")


def test_the_step_kernel_is_untouched():
    """raft_build_kernel_source_id() is unchanged from the parent commit: the
    step kernel's sources (build.py KERNEL_SOURCES: raft_step.h, philox.h,
    raft_engine.hip, raft_engine_impl.h) are the parent's, byte for byte.  The
    outbox keeps its state in HBM behind the leader watch's pairs and owns no
    engine member."""
    assert abi.build_ids()["kernel_source_id"] == PARENT_KERNEL_SOURCE_ID
