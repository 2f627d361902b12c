"""Scripted network faults on the GPU (marker `gpu`): raft_isolate_batch*,
raft_engine_heal_network* and raft_engine_list_isolated* against the oracle
driven through tests/nemesis_model.py (read_state -> model -> write_state).
Every comparison is exact."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest

import nemesis_model as NM
import restart_model as RM
import transfer_model as TM
from helpers import STRESS_MIX, abi, fld

pytestmark = pytest.mark.gpu

eng_mod = importlib.import_module("raft-kotlin_amd.engine")
service = importlib.import_module("raft-kotlin_amd.service")
RaftEngine = eng_mod.RaftEngine
RaftError = eng_mod.RaftError

G = 70                                   # 64 // R groups a step-kernel wave: several waves and a ragged last one
RING_WINDOW = 32


def same(got, want, label=""):
    assert got.dtype == want.dtype and len(got) == len(want), (label, got.dtype, len(got), len(want))
    if not np.array_equal(got, want):
        at = int(np.nonzero(got != want)[0][0])
        raise AssertionError(f"{label}: {int((got != want).sum())} records differ; first at {at}: {got[at]} vs {want[at]}")


# ---- parity with the oracle
def parity_kw(R: int, mode: str, log: str, faults: str = "plain") -> dict:
    """plain: no churn and (at R = 5) no drops either, so before the first
    isolation the engine runs a kernel built without the isolation check and
    must switch; churn: the stress mix, where the harness isolates too."""
    kw = dict(R=R, G=G, seed=11, log_cap=300, cmd_ppm=500_000, drop_ppm=0 if R == 5 else 100_000)
    if faults != "plain":
        kw.update(STRESS_MIX)
    if faults == "general":
        kw["kernel"] = abi.KERNEL_GENERAL
    if mode == "textbook":
        kw.update(mode=abi.MODE_TEXTBOOK, ae_max_entries=4)
    if log == "ring":
        # a replica cut off for up to 44 steps at a command every other step falls 22 entries and more behind: a
        # 16-slot window would lose them (the run would be invalid from there on); 32 slots hold them, and the
        # logs still grow past 32, so the ring wraps
        kw["log_window"] = RING_WINDOW
    return kw


def parity_messages(R: int):
    """One message per group of [2, G - 1) and 9 of them again: by index, by
    both leader selectors, 3..44 steps (some run out inside the 30 steps)."""
    g = np.arange(2, G - 1, dtype=np.int64)
    g = np.concatenate([g, g[::8]])
    t = np.where(g % 3 == 0, NM.NEWEST, np.where(g % 3 == 1, NM.LOWEST, g % R)).astype(np.int32)
    s = (3 + (g * 7) % 42).astype(np.int32)
    return g, t, s


def parity_run(x, label: str = "") -> list:
    """On `x` (a Host or a RaftEngine): 40 steps, an isolate batch, 30 steps, the
    batch again without and with REPLACE, 10 steps, a heal of replicas 0 and 2
    over [5, G - 3), the listing, 10 steps.  Returns the checkpoints."""
    out = []

    def snap(what, **more):
        out.append(dict(what=f"{label} {what}", state=x.read_state(), logs=x.read_log(), digest=x.digest(), **more))

    g, t, s = parity_messages(x.R)
    snap("warm-up", counters=x.step(40))
    snap("isolate", tickets=x.isolate(g, t, s))
    snap("cut", counters=x.step(30))
    snap("again", tickets=x.isolate(g, t, s))
    snap("replace", tickets=x.isolate(g, t, s, replace=True))
    snap("cut again", counters=x.step(10))
    snap("heal", info=x.heal_network(np.full(G - 8, 0b101, np.uint8), g0=5))
    info, rec = x.isolated()
    snap("list", info=info, tickets=rec)
    snap("run-on", counters=x.step(10))
    return out


PARITY_CASES = [(R, mode, log, "plain") for R in (3, 5, 8) for mode in ("reference", "textbook")
                for log in ("flat", "ring")] + [(5, "reference", "flat", "churn"), (5, "reference", "flat", "general")]


@functools.lru_cache(maxsize=None)
def host_parity_run(R, mode, log, faults):
    h = NM.Host(0, **parity_kw(R, mode, log, faults))
    points = parity_run(h, f"R{R} {mode} {log} {faults}")
    h.close()
    return points


@pytest.mark.parametrize("R,mode,log,faults", PARITY_CASES, ids=["-".join(map(str, c)) for c in PARITY_CASES])
def test_parity_with_the_oracle(R, mode, log, faults):
    """Tickets, infos, the listing, state, logs, digest and counter rows equal
    the oracle's under the model at every checkpoint, bit for bit."""
    want = host_parity_run(R, mode, log, faults)
    st = {p["what"].split(" ", 4)[-1]: p for p in want}
    first = st["isolate"]["tickets"]["status"]
    assert (first == NM.SET).sum() > 0 and (first == NM.DUPLICATE).sum() == 9
    assert (st["again"]["tickets"]["status"] == NM.BUSY).sum() > 0
    if faults != "plain":                                            # a harness isolation met: BUSY, then overwritten
        met, later = (first == NM.BUSY), st["replace"]["tickets"]["status"]
        assert met.sum() > 0 and (later[met] == NM.SET).sum() > 0 and (later != NM.BUSY).all()
    assert st["heal"]["info"]["healed"] > 0 and st["heal"]["info"]["kept"] > 0 and st["list"]["info"]["running"] > 0
    # the oracle's run is valid to its last step (on a ring: no access below a window), so assert_same_points
    # compares every checkpoint; and a ring case does wrap
    rows = np.concatenate([p["counters"] for p in want if "counters" in p])
    assert len(rows) == 90 and RM.valid_rows(rows) == 90 and rows[:, abi.C_INDEX["log_window_miss"]].sum() == 0
    if log == "ring":
        assert max(int(fld(want[-1]["state"], R, r, "phys").max()) for r in range(R)) > RING_WINDOW
    with RaftEngine(abi.make_params(**parity_kw(R, mode, log, faults))) as e:
        got = parity_run(e, f"R{R} {mode} {log} {faults}")
    TM.assert_same_points(got, want, R)


# ---- tickets against the model
@functools.lru_cache(maxsize=None)
def warm_state(R: int = 5):
    """The oracle's state after 40 steps of the churn mix (some groups have a
    harness isolation running, some have no leader, some two)."""
    h = NM.Host(0, **parity_kw(R, "reference", "flat", "churn"))
    h.step(40)
    st, logs = h.read_state(), h.read_log()
    h.close()
    return st, logs


@pytest.fixture(scope="module")
def engine():
    with RaftEngine(abi.make_params(**parity_kw(5, "reference", "flat", "churn"))) as e:
        yield e


def load(e, st=None):
    st0, logs = warm_state()
    e.write_log(*logs)
    e.write_state(st0 if st is None else st)
    return st0.copy()


@pytest.mark.parametrize("n", [1, 64, 65, 257, 1000])
@pytest.mark.parametrize("replace", [False, True])
def test_tickets_equal_the_model(engine, n, replace):
    """Batches with many messages per group (1000 over 70 groups), up to a
    wave, one past it, past a workgroup: every ticket and the state afterwards
    equal the model's -- and again with the batch reversed, against the model of
    the reversed batch."""
    e = engine
    groups, targets, steps = NM.contended_batch(G, 5, n)
    for tag, sl in (("forward", slice(None)), ("reversed", slice(None, None, -1))):
        g, t, s = (np.ascontiguousarray(a[sl]) for a in (groups, targets, steps))
        model = load(e)
        want, rc = NM.isolate(model, g, t, s, 5, replace)
        assert rc == abi.RAFT_OK
        same(e.isolate(g, t, s, replace=replace), want, f"n={n} {tag}")
        assert np.array_equal(e.read_state(), model), f"n={n} {tag}: the state differs from the model's"
    if n == 1000:
        assert {NM.SET, NM.DUPLICATE, NM.INVALID, NM.NO_LEADER} <= set(want["status"].tolist())
        assert replace or NM.BUSY in want["status"]


def test_crafted_statuses_on_the_device():
    w, tgt, stp, want, forced = NM.crafted()
    n = len(NM.CRAFTED_NAMES)
    with RaftEngine(abi.make_params(R=NM.CR, G=n, log_cap=8)) as e:
        for replace, exp in ((False, want), (True, forced)):
            e.write_state(w)
            model = w.copy()
            NM.isolate(model, np.arange(n), tgt, stp, NM.CR, replace)
            same(e.isolate(np.arange(n), tgt, stp, replace=replace), exp, f"crafted replace={replace}")
            assert np.array_equal(e.read_state(), model)
        # positions 5, 2 and 9 to one group: 2 wins, the others name 2
        e.write_state(w)
        groups = np.array([0, 3, 3, 1, 2, 3, 4, 5, 6, 3], dtype=np.int64)
        targets = np.array([0, NM.CR, 2, 0, 0, 4, 0, 0, 0, 1], dtype=np.int32)
        steps = np.array([5, 5, 6, 5, 5, 7, 5, 5, 5, 8], dtype=np.int32)
        tk = e.isolate(groups, targets, steps)
        assert tk[[1, 2, 5, 9]].tolist() == [(-1, 5, NM.INVALID, 0), (2, 6, NM.SET, 0), (-1, 7, NM.DUPLICATE, 2),
                                             (-1, 8, NM.DUPLICATE, 2)]
        assert e.read_state()[3, NM.ISO] == 6 << 8 | 2


# ---- the _dev forms, heal, list
def test_host_and_device_buffers_agree():
    """The host forms and the _dev forms on two engines in the same state give
    identical tickets, infos, records and digests, and the _dev forms write
    nothing beyond their records."""
    import torch
    kw = parity_kw(5, "reference", "flat", "churn")
    g, t, s = NM.contended_batch(G, 5, 300, seed=1)
    n = len(g)
    mask = np.full(G - 8, 0b01101, np.uint8)
    with RaftEngine(abi.make_params(**kw)) as a, RaftEngine(abi.make_params(**kw)) as b:
        for e in (a, b):
            load(e)
        tk = a.isolate(g, t, s, replace=True)
        dg, dt, ds = (torch.from_numpy(x).to("cuda:0") for x in (g, t, s))
        dk = torch.full(((n + 1) * 4,), -7, dtype=torch.int32, device="cuda:0")
        dm = torch.from_numpy(mask).to("cuda:0")
        torch.cuda.synchronize()
        assert b.isolate_dev(dg.data_ptr(), dt.data_ptr(), ds.data_ptr(), dk.data_ptr(), n, replace=True) == abi.RAFT_OK
        raw = dk.cpu().numpy()
        same(raw[:-4].view(abi.ISOLATE_TICKET_DTYPE), tk, "device tickets")
        assert (raw[-4:] == -7).all() and (tk["status"] == NM.SET).sum() > 0
        assert a.digest() == b.digest()
        info, rec = a.isolated()
        k = info["running"]
        assert k > 2 and info == dict(delivered=k, pending=0, running=k)
        dr = torch.full(((k + 1) * 4,), -7, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        assert b.isolated_dev(dr.data_ptr(), k) == info
        raw = dr.cpu().numpy()
        same(raw[:-4].view(abi.ISOLATED_DTYPE), rec, "device records")
        assert (raw[-4:] == -7).all()
        hi = a.heal_network(mask, g0=5)
        assert b.heal_network_dev(dm.data_ptr(), len(mask), g0=5) == hi and hi["healed"] > 0 and hi["kept"] > 0
        assert a.digest() == b.digest()
        assert b.heal_network_dev(0, G) == a.heal_network() and a.digest() == b.digest()
        assert a.isolated()[0] == dict(delivered=0, pending=0, running=0)


def test_heal_with_and_without_a_mask(engine):
    e = engine
    model = load(e)
    g = np.arange(G, dtype=np.int64)
    NM.isolate(model, g, g % 5, 9, 5, True)
    e.isolate(g, g % 5, 9, replace=True)
    mask = np.where(np.arange(G - 10) % 2 == 0, 0b00110, 0xE0).astype(np.uint8)   # bits at or above R select nothing
    want = NM.heal(model, 5, mask, g0=4)
    assert e.heal_network(mask, g0=4) == want and want["healed"] > 0 and want["kept"] > 0 and want["idle"] == 0
    assert np.array_equal(e.read_state(), model)
    assert e.heal_network(g0=60, n=10) == NM.heal(model, 5, None, 60, 10) and np.array_equal(e.read_state(), model)
    want = NM.heal(model, 5)
    assert e.heal_network() == want and want["idle"] > 0 and (e.read_state()[:, NM.ISO] == 0).all()
    assert e.heal_network(np.zeros(0, np.uint8)) == dict(healed=0, idle=0, kept=0)


def test_list_cut_and_peek(engine):
    e = engine
    model = load(e)
    g = np.arange(3, G, 2, dtype=np.int64)
    for x in (lambda *a: NM.isolate(model, *a, 5, True), lambda *a: e.isolate(*a, replace=True)):
        x(g, NM.LOWEST, 11)
    _, full = NM.list_isolated(model, 5)
    k = len(full)
    assert k >= 10
    before = e.digest()
    assert e.isolated(peek=True)[0] == dict(delivered=0, pending=k, running=k)
    for room in (0, 1, k - 1, k, k + 5):
        info, rec = e.isolated(max_events=room)
        want_info, want = NM.list_isolated(model, 5, max_events=room)
        assert info == want_info
        same(rec, want, f"room {room}")
        if 0 < room < k:                                             # the rest, from the group after the cut
            nxt = int(rec["group"][-1]) + 1
            same(np.concatenate([rec, e.isolated(g0=nxt)[1]]), full, f"room {room} and the rest")
    info, rec = e.isolated(g0=20, n=33)
    want_info, want = NM.list_isolated(model, 5, 20, 33)
    assert info == want_info and 0 < len(want) < k
    same(rec, want, "a sub-range")
    assert e.digest() == before                                      # read-only


def test_a_transfer_to_an_isolated_target_is_unreachable():
    R, n, cap = 5, 8, 8
    w, _ = TM.healthy(n, R)
    terms = np.zeros((n, R, cap), np.int32)
    terms[:, :, :3], terms[:, :, 3] = 1, 2
    with RaftEngine(abi.make_params(R=R, G=n, log_cap=cap, mode=1)) as e:
        e.write_state(w)
        e.write_log(terms, np.zeros((n, R, cap), np.uint32))
        even = np.arange(0, n, 2, dtype=np.int64)
        assert (e.isolate(even, 2, 5)["status"] == NM.SET).all()
        tk = e.transfer(np.arange(n), np.full(n, 2, np.int32))
        assert tk["status"][0::2].tolist() == [TM.UNREACHABLE] * (n // 2)
        assert tk["status"][1::2].tolist() == [TM.SENT] * (n // 2)
        svc = service.RaftService(e)
        assert svc.transfer_leadership(0, 2) == "UNREACHABLE"
        assert [(x.group, x.replica, st, rem) for x, st, rem in svc.isolated()] == [(int(g), 2, "FOLLOWER", 5) for g in even]
        assert svc.node(1, 3).isolate(4) == "SET" and svc.node(1, 4).isolate(4) == "BUSY"
        assert svc.isolate([3, 5], "leader", 6)["replica"].tolist() == [1, 1]
        assert svc.heal_network() == dict(healed=n // 2 + 3, idle=n // 2 - 3, kept=0)
        assert svc.transfer_leadership(0, 2) == "SENT"


def test_call_errors(engine):
    """A null array with n > 0, n < 0, unknown flags and a group outside the
    engine: refused, and the engine's state is unchanged by digest."""
    e = engine
    load(e)
    before = e.digest()
    with pytest.raises(RaftError, match="outside the engine"):
        e.isolate(np.arange(G + 1), 0, 5)
    with pytest.raises(RaftError, match="outside the engine"):
        e.isolate([5, -1], [0, 0], 5)
    for g0, n in ((G, 1), (-1, 2), (G - 1, 2)):
        with pytest.raises(RaftError, match="outside the engine"):
            e.heal_network(g0=g0, n=n)
        with pytest.raises(RaftError, match="outside the engine"):
            e.isolated(g0=g0, n=n)
    lib, h = e._lib, e._h
    buf = np.zeros(64, np.int64)
    p = C.c_void_p(buf.ctypes.data)
    hi, li = abi.raft_heal_info(), abi.raft_isolated_info()
    hi.healed = li.running = 5
    assert lib.raft_isolate_batch(h, None, None, None, 0, None, 0) == abi.RAFT_OK
    assert lib.raft_engine_heal_network(h, G, 0, None, C.byref(hi)) == abi.RAFT_OK and hi.healed == 0
    assert lib.raft_engine_list_isolated(h, G, 0, None, 0, C.byref(li)) == abi.RAFT_OK and li.running == 0
    assert len(e.isolate([], [], [])) == 0
    for fn in (lib.raft_isolate_batch, lib.raft_isolate_batch_dev):
        for args in ((None, p, p, 0, p), (p, None, p, 0, p), (p, p, None, 0, p), (p, p, p, 0, None)):
            assert fn(h, *args, 1) == abi.RAFT_EINVAL
        assert fn(h, p, p, p, 0, p, -1) == abi.RAFT_EINVAL
        assert fn(h, p, p, p, 2, p, 1) == abi.RAFT_EINVAL
    assert lib.raft_engine_heal_network(h, 0, 4, None, None) == abi.RAFT_EINVAL
    assert lib.raft_engine_list_isolated(h, 0, 4, None, 0, None) == abi.RAFT_EINVAL
    assert lib.raft_engine_list_isolated(h, 0, 4, None, 3, C.byref(li)) == abi.RAFT_EINVAL
    assert lib.raft_engine_list_isolated(h, 0, 4, p, -1, C.byref(li)) == abi.RAFT_EINVAL
    assert lib.raft_engine_list_isolated_dev(h, 0, 4, C.c_void_p(buf.ctypes.data + 8), 1, C.byref(li)) == abi.RAFT_EINVAL
    assert e.digest() == before
