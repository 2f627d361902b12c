"""The liveness monitor on the CPU: tests/monitor_model.py (the numpy
restatement of include/raft_engine.h raft_monitor_*) on hand-written groups --
one per rule and per non-case -- and over the oracle: the counter identity
with RAFT_C_GROUPS_WITH_LEADER, and a sampled run against a scalar
re-derivation.  No device is touched; test_gpu_monitor.py holds the engine's
kernels to the same model."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest

import monitor_model as MM
import restart_model as RM
from helpers import STRESS_MIX, abi, fld

engine_mod = importlib.import_module("raft-kotlin_amd.engine")
service_mod = importlib.import_module("raft-kotlin_amd.service")


def run_crafted():
    """The three crafted phases from crafted_ledger0: (the ledger after each, the infos, the totals)."""
    L, av = MM.crafted_ledger0(), MM.zero_avail()
    out, infos = [], []
    for k in range(3):
        info, rc = MM.observe(MM.crafted_phase(k), L, av, MM.CRAFTED_CFG, MM.CR, MM.CCAP, MM.CRAFTED_STEPS[k])
        assert rc == abi.RAFT_OK
        out.append(L.copy())
        infos.append(info)
    return out, infos, av


def test_abi_names_the_monitor():
    """The pieces a caller needs exist (they do not on a tree without the monitor)."""
    assert abi.MONITOR_WORDS == 16 == len(abi.MONITOR_WORD_NAMES) and abi.MONITOR_EVENT_DTYPE.itemsize == 32
    assert C.sizeof(abi.raft_monitor_config) == 32 and C.sizeof(abi.raft_monitor_info) == 96
    assert C.sizeof(abi.raft_monitor_event) == 32 and C.sizeof(abi.raft_monitor_report_info) == 64
    assert C.sizeof(abi.raft_monitor_availability) == 288
    assert len(abi.MONITOR_INFO_FIELDS) == 10 and abi.MONITOR_KINDS == ("leaderless", "commit_stalled", "lagging", "churning")
    assert hasattr(engine_mod.RaftEngine, "monitor") and hasattr(engine_mod, "RaftMonitor")
    for name in ("observe", "report", "report_dev", "read", "write", "reset", "availability", "set_availability",
                 "device_bytes", "close"):
        assert hasattr(engine_mod.RaftMonitor, name), name
    for name in ("check_liveness", "unavailable", "remediate"):
        assert hasattr(service_mod.RaftService, name), name
    assert {n for n in abi.EXPORTED_SYMBOLS if n.startswith("raft_monitor_")} == {
        "raft_monitor_create", "raft_monitor_destroy", "raft_monitor_reset", "raft_monitor_device_bytes",
        "raft_monitor_observe", "raft_monitor_report", "raft_monitor_report_dev", "raft_monitor_get_availability",
        "raft_monitor_set_availability", "raft_monitor_read", "raft_monitor_write"}


def test_one_group_per_rule_and_per_non_case():
    """monitor_model.CRAFTED: no leader below, at and above leaderless_steps;
    outages of length 1, 4 and 10 in buckets 0, 2 and 3; a stale leader beside a
    newer one; a backlog that advances, one that does not, a new leader below
    the mark, a backlog that disappears; a lag one below lag_entries and at it;
    a lagging stale leader; a churn window that rolls over; a step index that
    went backwards.  The now and ever words are the hand-written ones."""
    ledgers, infos, av = run_crafted()
    for k in range(3):
        for word, want in ((MM.NOW, MM.crafted_now(k)), (MM.EVER, MM.crafted_ever(k))):
            got = ledgers[k][:, word]
            assert np.array_equal(got, want), (k, word, [(n, int(a), int(b)) for n, a, b in
                                                         zip(MM.CRAFTED_NAMES, got, want) if a != b])
    for name, words in MM.CRAFTED_WORDS.items():
        row = ledgers[2][MM.CRAFTED_NAMES.index(name)]
        assert {w: int(row[w]) for w in words} == words, name
    assert MM.same_avail(av, MM.crafted_avail()), av
    prev = np.zeros(len(MM.CRAFTED_NAMES), np.int32)
    for k in range(3):
        now = MM.crafted_now(k)
        assert infos[k]["flagged"] == int((now != 0).sum())
        assert infos[k]["newly_flagged"] == int(((prev == 0) & (now != 0)).sum())
        assert infos[k]["cleared"] == int(((prev != 0) & (now == 0)).sum())
        for kind, bit in MM.BITS.items():
            assert infos[k][kind] == int(((now & bit) != 0).sum()), (k, kind)
        prev = now
    assert [i["outages_ended"] for i in infos] == [1, 1, 1] and [i["down_steps_ended"] for i in infos] == [1, 4, 10]
    assert [i["down"] for i in infos] == [4, 3, 2]     # down_all and backwards; outage_mid till 14, outage_long till 20
    # every bit is covered by some group, the non-cases stay clean, something cleared
    assert np.bitwise_or.reduce(MM.crafted_ever(2)) == abi.MONITOR_ALL and (MM.crafted_ever(2) == 0).sum() >= 5
    assert infos[2]["cleared"] == 3
    # the reports: now against ever, the kinds filter, a cut
    L = ledgers[2]
    info, ev, rc = MM.report(L)
    assert rc == abi.RAFT_OK and ev["group"].tolist() == np.nonzero(MM.crafted_now(2))[0].tolist()
    info, ev, rc = MM.report(L, ever=True)
    assert ev["group"].tolist() == np.nonzero(MM.crafted_ever(2))[0].tolist() and info["pending"] == 0
    _, only, _ = MM.report(L, ever=True, kinds=MM.LAG)
    assert [MM.CRAFTED_NAMES[g] for g in only["group"]] == ["lag_edge", "lag_stale_leader"]
    assert only["lag_mask"].tolist() == [0, 1] and only["leader"].tolist() == [0, 1]
    cut, ev2, _ = MM.report(L, ever=True, max_events=2)
    assert cut == dict(delivered=2, pending=len(ev) - 2, flagged=len(ev)) and np.array_equal(ev2, ev[:2])
    assert MM.report(L, kinds=16)[2] == abi.RAFT_EINVAL and MM.report(L, 0, len(L) + 1)[2] == abi.RAFT_ERANGE


def test_bulk_groups_show_every_kind():
    """monitor_model.bulk (the G = 70,001 case of test_gpu_monitor.py, here at 203)."""
    p0, p1, want = MM.bulk(203)
    L, av = MM.fresh(203), MM.zero_avail()
    i0, _ = MM.observe(p0, L, av, MM.BULK_CFG, 3, 16, MM.BULK_STEPS[0])
    assert i0["flagged"] == 0 and i0["down"] == 2                      # groups 10 and 110
    i1, _ = MM.observe(p1, L, av, MM.BULK_CFG, 3, 16, MM.BULK_STEPS[1])
    assert np.array_equal(L[:, MM.NOW], want)
    # two groups of each of the five kinds; the fifth carries three bits
    assert (i1["leaderless"], i1["commit_stalled"], i1["lagging"], i1["churning"]) == (2, 4, 4, 4) and i1["flagged"] == 10


def test_write_reset_and_config_rules():
    R = 3
    ok = MM.fresh(4)
    assert MM.valid_ledger(ok, R)
    for word, v in ((MM.NOW, 16), (MM.NOW, -1), (MM.EVER, 32), (MM.LEADER, R), (MM.LEADER, -2), (MM.LAG_MASK, 1 << R),
                    (MM.LAG_MASK, -1), (MM.OUTAGES, -1), (MM.DOWN_TOTAL, -1), (MM.LONGEST, -5), (MM.MAX_LAG, -1),
                    (MM.STALL_MARK, -1), (MM.RSV0, 1), (MM.RSV1, -1)):
        bad = ok.copy()
        bad[2, word] = v
        assert not MM.valid_ledger(bad, R), (word, v)
    edge = ok.copy()
    edge[1, MM.NOW], edge[1, MM.EVER], edge[1, MM.LEADER], edge[1, MM.LAG_MASK] = 15, 15, R - 1, (1 << R) - 1
    edge[1, [MM.FIRST, MM.DOWN_SINCE, MM.STALL_SINCE, MM.WIN_START, MM.WIN_TERM]] = -7           # never an index
    edge[1, [MM.OUTAGES, MM.DOWN_TOTAL, MM.LONGEST, MM.MAX_LAG, MM.STALL_MARK]] = 2 ** 31 - 1
    assert MM.valid_ledger(edge, R)
    # the zero state is what the header's table says
    z = MM.fresh(1)[0]
    assert z.tolist() == [0, 0, 0, -1, -1, 0, 0, 0, -1, 0, -1, 0, 0, 0, 0, 0]
    assert MM.valid_config(MM.config()) and MM.valid_config(MM.CRAFTED_CFG)
    assert MM.valid_config(MM.config(churn_terms=0, churn_steps=0))
    for kw in (dict(leaderless_steps=-1), dict(stalled_steps=-1), dict(lag_entries=-2), dict(churn_terms=-1),
               dict(churn_steps=-1), dict(churn_terms=1, churn_steps=0)):
        assert not MM.valid_config(MM.config(**kw)), kw
    assert not MM.valid_config(MM.config(), reserved=(0, 1, 0))
    assert MM.valid_availability(np.zeros(32, np.int64), 0, 0)
    h = np.zeros(32, np.int64)
    h[31] = -1
    assert not MM.valid_availability(h, 0, 0) and not MM.valid_availability(np.zeros(32, np.int64), -1, 0)
    assert not MM.valid_availability(np.zeros(32, np.int64), 0, -1)
    # a saturated ledger stays saturated when one more outage ends
    L = MM.fresh(1)
    L[0, [MM.OUTAGES, MM.DOWN_TOTAL]] = 2 ** 31 - 1
    L[0, MM.DOWN_SINCE] = 3
    MM.observe(MM.build([MM._led], 3), L, MM.zero_avail(), MM.config(), 3, 16, 8)
    assert L[0, MM.OUTAGES] == L[0, MM.DOWN_TOTAL] == 2 ** 31 - 1 and L[0, MM.LONGEST] == 5


# ---- over the oracle
STEPS = 300
ORACLE_CASES = [(R, mode) for R in (3, 5) for mode in ("flat", "textbook")]


@functools.lru_cache(maxsize=None)
def oracle_run(R: int, mode: str):
    """300 faulted steps (helpers.STRESS_MIX, G = 203) on the oracle, the state's
    leader bit per group kept after every step, observed by two monitors with
    leaderless_steps = 0: after every step, and after every 7th."""
    kw = RM.parity_kw(R, 203, mode)
    assert all(kw[k] == v for k, v in STRESS_MIX.items())
    h = RM.Host(**kw)
    cfg = MM.config(leaderless_steps=0, stalled_steps=10, lag_entries=8, churn_terms=3, churn_steps=20)
    mon = {1: (MM.fresh(h.G), MM.zero_avail()), 7: (MM.fresh(h.G), MM.zero_avail())}
    leaderless, with_leader, led, infos7 = [], [], [], []
    for t in range(1, STEPS + 1):
        row = h.step(1)[-1]
        st = h.read_state()
        with_leader.append(int(row[abi.C_INDEX["groups_with_leader"]]))
        led.append(np.stack([fld(st, R, r, "role") == abi.LEADER for r in range(R)], 1).any(axis=1))
        for k, (L, av) in mon.items():
            if t % k == 0:
                info, rc = MM.observe(st, L, av, cfg, R, h.cap, h.step_index)
                assert rc == abi.RAFT_OK and h.step_index == t
                (leaderless if k == 1 else infos7).append(info)
    h.close()
    return dict(G=203, mon=mon, leaderless=leaderless, with_leader=with_leader, led=np.array(led), infos7=infos7)


@pytest.mark.parametrize("R,mode", ORACLE_CASES)
def test_counter_identity_on_the_oracle(R, mode):
    """Observed after every step with leaderless_steps = 0: info.leaderless is
    G - RAFT_C_GROUPS_WITH_LEADER of that step; at the end the ended outages'
    lengths plus the running ones' add up to the steps the counter says groups
    spent without a leader; the histogram counts every ended outage.  A
    running outage first seen at step a has shown no leader at the observes
    a .. STEPS, one more than age(down_since) = STEPS - a at the last of them: its
    length so far is its age one step on, which is what an ending there would
    record.  (With the ages taken at STEPS itself the two sides differ by exactly
    the number of running outages: 127, 69, 159 and 93 in the four runs here.)"""
    run = oracle_run(R, mode)
    G = run["G"]
    L, av = run["mon"][1]
    got = [i["leaderless"] for i in run["leaderless"]]
    want = [G - c for c in run["with_leader"]]
    assert got == want, next((t, a, b) for t, (a, b) in enumerate(zip(got, want)) if a != b)
    assert [i["down"] for i in run["leaderless"]] == want              # at 0 steps every down group is flagged
    running = L[:, MM.DOWN_SINCE] != -1
    ages = int(MM.age(STEPS, L[running, MM.DOWN_SINCE].astype(np.int64)).sum())
    so_far = int(MM.age(STEPS + 1, L[running, MM.DOWN_SINCE].astype(np.int64)).sum())
    print(f"R{R} {mode}: down_total {int(L[:, MM.DOWN_TOTAL].sum())}, running outages {int(running.sum())} of ages {ages}, "
          f"leaderless group-steps {sum(want)}")
    assert so_far == ages + int(running.sum())
    assert int(L[:, MM.DOWN_TOTAL].sum()) + so_far == sum(want)
    assert int(av["hist"].sum()) == int(L[:, MM.OUTAGES].sum()) == av["outages"] > 0
    assert av["down_steps"] == int(L[:, MM.DOWN_TOTAL].sum())
    assert sum(i["outages_ended"] for i in run["leaderless"]) == av["outages"]
    assert (L[:, MM.EVER] & MM.LL).all()                                # every group waited for its first leader


@pytest.mark.parametrize("R,mode", ORACLE_CASES)
def test_sampled_every_7_steps_against_a_scalar_rederivation(R, mode):
    """The same run observed after every 7th step: outages, longest,
    down_total, down_since and the histogram are those of the sampled sequence
    of "some replica is LEADER", re-derived per group in plain Python."""
    run = oracle_run(R, mode)
    L, av = run["mon"][7]
    led = run["led"]                                                    # [step - 1, group]
    hist = np.zeros(abi.MONITOR_HIST, np.int64)
    for g in range(run["G"]):
        ended, since = MM.outages_of([(t, bool(led[t - 1, g])) for t in range(7, STEPS + 1, 7)])
        assert int(L[g, MM.OUTAGES]) == len(ended) and int(L[g, MM.DOWN_TOTAL]) == sum(ended), g
        assert int(L[g, MM.LONGEST]) == max(ended, default=0), g
        assert int(L[g, MM.DOWN_SINCE]) == (-1 if since is None else since), g
        for ln in ended:
            hist[ln.bit_length() - 1] += 1
    assert np.array_equal(av["hist"], hist) and av["outages"] == int(hist.sum()) > 0
    assert av["down_steps"] == int(L[:, MM.DOWN_TOTAL].sum())
    assert (L[:, MM.LONGEST] % 7 == 0).all()                            # sampled instants: lengths in units of 7
    # the sampled monitor sees fewer, longer outages than the one that looks after every step
    assert av["outages"] < run["mon"][1][1]["outages"]
    assert sum(i["outages_ended"] for i in run["infos7"]) == av["outages"]
