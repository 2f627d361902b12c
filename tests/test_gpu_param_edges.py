"""The raft_params corners and the state-restore entry points on the GPU
(marker `gpu`): the Philox key's high word, global group ids with bit 31 set,
step indices up to and across the 32-bit wrap, checkpoint and resume through
write_state / write_log / set_step_index, non-default timer constants and the
ends of the fault rates -- everywhere bit-exact against the CPU oracle
(per-step counters, canonical state, logs, digest), on the automatic kernel
and schedule, on the forced balanced schedule and on the general kernel.

Sizes: 1,500 groups (1,501 at R = 5) are 72 / 126 / 167 chunks of 64 // R
groups, the last one part-full at every R; 300 steps reach elections, commits
and every fault of the stress mix (assert_not_vacuous on the oracle's rows).
tests/test_param_edges_cpu.py runs the same parameter sets on the two CPU
implementations against each other."""
import collections
import importlib
import os

import numpy as np
import pytest

import oracle as O
from helpers import (DEGENERATE_TIMERS, FAULT_EDGES, SEEDS64, STRESS_MIX, TIMER_SETS, abi, assert_not_vacuous,
                     assert_same_logs, assert_same_state, fld, high_g0)
from test_gpu_parity import handler_messages, random_states

pytestmark = pytest.mark.gpu

eng_mod = importlib.import_module("raft-kotlin_amd.engine")
RaftEngine = eng_mod.RaftEngine

NTHREADS = min(16, os.cpu_count() or 1)
STEPS, CAP = 300, 300
# A 64-slot ring under the stress mix: from about step 210 on a replica that a
# partition or an isolation left far behind makes its leader read below the
# window (RAFT_C_LOG_WINDOW_MISS; such a run is not the reference's, and the
# oracle serves the read where a ring cannot).  The ring cases stop at 200
# steps, with the rings wrapped (physLen ~ 85 > 64) and no miss: both asserted.
RING_STEPS = 200
VARIANTS = ["auto", "balanced", "general"]
C = abi.C_INDEX

Run = collections.namedtuple("Run", "counters state logs digest step_index")


def groups(R):
    return 1501 if R == 5 else 1500        # 64 // R groups per chunk: the last chunk part-full at R = 3, 5, 7


def stress(R=5, **kw):
    return dict(dict(R=R, G=groups(R), seed=21, log_cap=CAP, **STRESS_MIX), **kw)


class OracleRuns:
    """The oracle's run of a parameter set (from step index t0), computed once
    and shared by the kernel variants that follow each other; the last few are
    kept (a run's logs are ~20 MB)."""

    def __init__(self):
        self.kept = collections.OrderedDict()

    def __call__(self, kw, steps=STEPS, t0=None, vacuous_ok=False):
        key = (tuple(sorted(kw.items())), steps, t0)
        if key not in self.kept:
            o = O.Oracle(abi.make_params(**kw))
            if t0 is not None:
                o.step_index = t0
            co = o.step(steps, nthreads=NTHREADS)[:, : abi.NUM_COUNTERS].copy()
            self.kept[key] = Run(co, o.read_state(), o.read_log(), o.digest(), o.step_index)
            o.close()
            while len(self.kept) > 3:
                self.kept.popitem(last=False)
        run = self.kept[key]
        if not vacuous_ok:
            assert_not_vacuous(run.counters, kw)
        return run


@pytest.fixture(scope="module")
def oracle_run():
    return OracleRuns()


def make_engine(kw, variant, **over):
    """The engine of a kernel variant: the automatic kernel and schedule (one
    launch of up to 400 steps), the balanced schedule forced on 7 workgroups
    with 37-step launches, or the general (NET_ALL) kernel in 64-step launches."""
    extra = {"auto": dict(steps_per_launch=abi.BENCH_STEPS_PER_LAUNCH),
             "balanced": dict(schedule=abi.SCHED_BALANCED, schedule_workgroups=7, steps_per_launch=37),
             "general": dict(steps_per_launch=64)}[variant]
    e = RaftEngine(abi.make_params(**dict(kw, **dict(extra, **over))))
    if variant == "general":
        e.set_kernel(abi.KERNEL_GENERAL)
    return e


def expected_net(kw, iso_written=False):
    return abi.step_net(kw["R"], kw.get("drop_ppm", 0), kw.get("partition_period", 0), kw.get("partition_len", 0),
                        kw.get("churn_ppm", 0), iso_written=iso_written,
                        cmd_mode=kw.get("cmd_mode", abi.CMD_LOWEST_LEADER), cmd_limit=kw.get("cmd_limit", 0))


def check_kernel(e, kw, variant, iso_written=False):
    """The last launch ran the kernel and schedule the variant names: no case
    falls back to another one unnoticed."""
    info = e.kernel_info()
    assert info["textbook"] == (kw.get("mode", 0) == abi.MODE_TEXTBOOK) and info["ring"] == (kw.get("log_window", 0) != 0)
    if variant == "general":
        assert info["net"] == abi.NET_ALL and info["balanced"] == 0, info
    elif variant == "balanced":
        assert info["net"] == expected_net(kw, iso_written) and info["balanced"] == info["subranges"] >= 1, info
    else:
        assert info["net"] == expected_net(kw, iso_written) and info["balanced"] == 0, info


def assert_wrapped_without_a_miss(run, R, window=64):
    assert run.counters[:, C["log_window_miss"]].sum() == 0, "a window miss: the run is not the reference's"
    assert max(int(fld(run.state, R, r, "phys").max()) for r in range(R)) > window, "the rings must have wrapped"


def same_counters(ce, co, label, first=0):
    if not np.array_equal(ce, co):
        bad = np.argwhere(ce != co)[0]
        raise AssertionError(f"{label}: counters differ at step {first + bad[0]} ({abi.COUNTER_NAMES[bad[1]]}): "
                             f"{ce[tuple(bad)]} vs {co[tuple(bad)]}")


def check_final(e, run, R, label):
    se = e.read_state()
    assert_same_state(se, run.state, R, label)
    assert_same_logs(se, e.read_log(), run.logs, R, label)
    assert e.digest() == run.digest, f"{label}: digest differs with equal state and logs"
    assert e.step_index == run.step_index, f"{label}: step index {e.step_index} vs the oracle's {run.step_index}"


def check_variant(kw, variant, run, label, t0=None):
    """A whole run of the variant's engine against the oracle's."""
    e = make_engine(kw, variant)
    try:
        if t0 is not None:
            e.step_index = t0
        ce = e.step(len(run.counters))
        check_kernel(e, kw, variant)
        same_counters(ce, run.counters, label)
        check_final(e, run, kw["R"], label)
    finally:
        e.close()


# ---- a. 64-bit seeds --------------------------------------------------------------

SEED_IDS = ["all64", "hi+7", "lo7"]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("R", [3, 5, 7])
@pytest.mark.parametrize("seed", SEEDS64, ids=SEED_IDS)
def test_seed_64_bit(oracle_run, R, seed, variant):
    """DevParams::key1 != 0: the odd Philox round keys of kdraw."""
    kw = stress(R, seed=seed)
    check_variant(kw, variant, oracle_run(kw), f"seed {seed:#x} R={R} {variant}")


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("case", ["textbook", "ring"])
def test_seed_64_bit_textbook_and_ring(oracle_run, case, variant):
    kw = stress(5, seed=SEEDS64[0], **(dict(mode=abi.MODE_TEXTBOOK, ae_max_entries=4) if case == "textbook"
                                       else dict(log_window=64)))
    run = oracle_run(kw, steps=RING_STEPS if case == "ring" else STEPS)
    if case == "ring":
        assert_wrapped_without_a_miss(run, 5)
    check_variant(kw, variant, run, f"seed64 {case} {variant}")


@pytest.mark.parametrize("seed", SEEDS64, ids=SEED_IDS)
@pytest.mark.parametrize("g0", [0, (1 << 32) - 1000], ids=["g0=0", "g0=top"])
def test_init_state_matches_oracle_at_64_bit_seeds(seed, g0):
    """init_kernel's draw(): test_init_state_matches_oracle's comparison."""
    kw = dict(R=5, G=1000, g0=g0, seed=seed, log_cap=16)
    e, o = RaftEngine(abi.make_params(**kw)), O.Oracle(abi.make_params(**kw))
    assert_same_state(e.read_state(), o.read_state(), 5, "init")
    assert e.digest() == o.digest()
    e.close()


def test_seeds_that_share_key0_differ(oracle_run):
    """(0x9E3779B9 << 32) | 7 and 7: the same key0, another key1 -- another
    run on the engine, each the oracle's."""
    got = []
    for seed in SEEDS64[1:]:
        kw = stress(5, seed=seed)
        run = oracle_run(kw)
        e = make_engine(kw, "auto")
        ce = e.step(STEPS)
        same_counters(ce, run.counters, f"seed {seed:#x}")
        assert e.digest() == run.digest
        got.append((e.digest(), ce.tobytes()))
        e.close()
    assert got[0][0] != got[1][0] and got[0][1] != got[1][1]


# ---- b. high global ids -----------------------------------------------------------

@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("R", [3, 5, 7])
@pytest.mark.parametrize("where", ["top", "bit31"])
def test_high_global_ids(oracle_run, R, where, variant):
    """gid() = gg0 + j() with bit 31 set, up to 2^32 - 1 (the last group of the
    `top` shard), and a shard with ids on both sides of 2^31."""
    kw = stress(R, g0=high_g0(groups(R))[where])
    assert kw["g0"] + kw["G"] == 1 << 32 if where == "top" else kw["g0"] < 1 << 31 < kw["g0"] + kw["G"]
    check_variant(kw, variant, oracle_run(kw), f"g0 {where} R={R} {variant}")


@pytest.mark.parametrize("R", [3, 5, 7])
@pytest.mark.parametrize("where", ["top", "bit31"])
def test_high_global_ids_shard_invariance(oracle_run, R, where):
    """Two engines on [g0, g0 + 700) and [g0 + 700, g0 + G): their counter rows
    sum to the whole shard's and their digests to its digest mod 2^64."""
    kw = stress(R, g0=high_g0(groups(R))[where])
    run = oracle_run(kw)
    cs, ds = [], []
    for g0, n in ((kw["g0"], 700), (kw["g0"] + 700, kw["G"] - 700)):
        e = make_engine(dict(kw, g0=g0, G=n), "auto")
        cs.append(e.step(STEPS))
        ds.append(e.digest())
        lo = g0 - kw["g0"]
        assert_same_state(e.read_state(), run.state[lo:lo + n], R, f"shard at {g0:#x}")
        e.close()
    same_counters(cs[0] + cs[1], run.counters, f"shards {where} R={R}")
    assert (ds[0] + ds[1]) % (1 << 64) == run.digest


@pytest.mark.parametrize("where", ["top", "bit31"])
def test_vote_batch_at_high_global_ids(where):
    """2,000 random RequestVote messages on a shard of high ids, at a step
    index with bit 31 set: a vote that makes a FOLLOWER re-arms its election
    timer with a draw keyed by the global id (raft_batch.hip), on both batch
    paths, against the oracle's handler message by message."""
    R, G, cap, n = 5, 200, 8, 2000
    rng = np.random.default_rng(97)
    kw = dict(R=R, G=G, g0=high_g0(G)[where], log_cap=cap, seed=SEEDS64[0])
    w, lt, lc = random_states(rng, G, R, cap)
    grp, dst, vq, _, _ = handler_messages(rng, n, G, R, cap)
    o = O.Oracle(abi.make_params(**kw))
    o.write_state(w)
    o.write_log(lt, lc)
    o.step_index = (1 << 32) - 3
    vo = np.array([o.vote(int(g), int(d), *map(int, q)) for g, d, q in zip(grp, dst, vq)], dtype=np.int32)
    so = o.read_state()
    el = np.stack([fld(so, R, r, "election_ms") for r in range(R)], 1)
    assert np.count_nonzero(el != 0) > 100, "the batch must re-arm election timers (blank states have electionMs 0)"
    assert el[el != 0].min() >= abi.DEFAULTS["election_min_ms"]
    for path in (abi.BATCH_PATH_BUCKETED, abi.BATCH_PATH_SORTED):
        e = RaftEngine(abi.make_params(**kw))
        e.set_batch_path(path)
        e.write_state(w)
        e.write_log(lt, lc)
        e.step_index = (1 << 32) - 3
        ve = e.vote_batch(grp, dst, vq)
        assert np.array_equal(ve, vo), f"path {path}: vote responses differ"
        assert_same_state(e.read_state(), so, R, f"vote batch, path {path}")
        e.close()


def test_ids_beyond_32_bits_are_refused():
    with pytest.raises(eng_mod.RaftError, match=r"\(-1\).*2\^32"):
        RaftEngine(abi.make_params(R=5, G=1500, g0=(1 << 32) + 1 - 1500, log_cap=16))


# ---- c. high step indices and the 32-bit wrap --------------------------------------

@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("R", [3, 5, 7])
@pytest.mark.parametrize("t0", [(1 << 32) - 1000, (1 << 32) - 150], ids=["high", "wrap"])
def test_high_step_indices(oracle_run, R, t0, variant):
    """raft_engine_set_step_index near 2^32; `wrap` crosses it at step 150,
    inside a fused launch (37 steps, and one launch of 300) and inside a
    partition window (t % 40 < 10 from 2^32 - 16: the window's first step
    t - ph is on the other side).  The index is a uint32_t everywhere, as in
    the oracle: it goes on at 0."""
    kw = stress(R)
    run = oracle_run(kw, t0=t0)
    assert run.step_index == (t0 + STEPS) % (1 << 32)
    check_variant(kw, variant, run, f"t0 {t0:#x} R={R} {variant}", t0=t0)


# ---- d. checkpoint and resume --------------------------------------------------------

RESUME_CASES = {
    # name: (params, N1, N1 + N2)
    "flat": (stress(5), 170, STEPS),
    "ring": (stress(5, log_window=64), 170, RING_STEPS),
    "R7-in-partition": (stress(7), 165, STEPS),               # 165 % 40 = 5: inside a partition window
    "churn": (stress(5, churn_ppm=200_000), 170, STEPS),
    "cmd_limit": (stress(5, cmd_limit=30), 170, STEPS),
    "textbook": (stress(5, mode=abi.MODE_TEXTBOOK, ae_max_entries=4), 170, STEPS),
    "R3-no-faults": (dict(R=3, G=1500, seed=21, log_cap=CAP, cmd_ppm=500_000), 170, STEPS),
}


@pytest.mark.parametrize("case", sorted(RESUME_CASES))
def test_checkpoint_and_resume(oracle_run, case):
    """Engine A runs N1 steps; its read_state, read_log and step_index go
    into a fresh engine B of another launch length, schedule and sub-range
    count (write_state, write_log, set_step_index, in that order).  The
    restore rebuilds what the canonical export does not carry (the log-tail
    cache, the primary session's owner, the spill rows, the isolation flag of
    the kernel choice): B's digest equals A's at once, and both step on to the
    oracle's counter rows [N1, N1 + N2), final state, logs and digest."""
    kw, n1, total = RESUME_CASES[case]
    R, n2 = kw["R"], total - n1
    run = oracle_run(kw, steps=total)
    a = make_engine(kw, "auto")
    same_counters(a.step(n1), run.counters[:n1], f"{case}: A")
    st, lg = a.read_state(), a.read_log()
    b = make_engine(kw, "balanced", subranges=2)
    b.write_state(st)
    b.write_log(*lg)
    b.step_index = a.step_index
    assert b.step_index == n1 and b.digest() == a.digest()
    assert_same_state(b.read_state(), st, R, f"{case}: B restored")
    assert_same_logs(st, b.read_log(), lg, R, f"{case}: B restored")
    iso = bool(np.any(st[:, -2] != 0))
    if case == "churn":
        assert iso, "an exported isolation word must be non-zero"
    if case == "R7-in-partition":
        assert n1 % kw["partition_period"] < kw["partition_len"]
    for e, name in ((a, "A"), (b, "B")):
        same_counters(e.step(n2), run.counters[n1:], f"{case}: {name} resumed", n1)
        check_final(e, run, R, f"{case}: {name}")
    check_kernel(a, kw, "auto")
    check_kernel(b, kw, "balanced", iso_written=iso)
    assert b.kernel_info()["subranges"] == 2
    if case == "churn":
        assert b.kernel_info()["net"] & abi.NET_ISO
    if case == "R3-no-faults":
        assert a.kernel_info()["net"] == b.kernel_info()["net"] == abi.NET_PART
    if case == "ring":
        assert_wrapped_without_a_miss(run, R)
        assert max(int(fld(st, R, r, "phys").max()) for r in range(R)) > 64, "the exported rings must have wrapped"
    a.close()
    b.close()


@pytest.mark.parametrize("R", [3, 5, 7])
def test_partial_restore(R):
    """Groups [7, 37) -- aligned to no chunk of 21, 12 or 9 groups -- of
    another run (another seed, at its step 170) written into an engine at step
    170, and into the oracle: read_state / read_log at that offset return what
    was written, and 130 more steps agree everywhere."""
    kw, kw2 = stress(R), stress(R, seed=22)
    e, d = make_engine(kw, "auto"), make_engine(kw2, "auto")
    o, od = O.Oracle(abi.make_params(**kw)), O.Oracle(abi.make_params(**kw2))
    for x in (e, d):
        x.step(170)
    for x in (o, od):
        x.step(170, nthreads=NTHREADS)
    st, lg = d.read_state(7, 30), d.read_log(7, 30)
    assert_same_state(st, od.read_state(7, 30), R, "the donor's export")
    assert_same_logs(st, lg, od.read_log(7, 30), R, "the donor's export")
    before = e.read_state()
    for x in (e, o):
        x.write_state(st, 7)
        x.write_log(*lg, 7)
    assert_same_state(e.read_state(7, 30), st, R, "read back")
    assert_same_logs(st, e.read_log(7, 30), lg, R, "read back")
    after = e.read_state()
    assert np.array_equal(after[:7], before[:7]) and np.array_equal(after[37:], before[37:])
    assert e.digest() == o.digest()
    ce = e.step(130)
    co = o.step(130, nthreads=NTHREADS)[:, : abi.NUM_COUNTERS]
    same_counters(ce, co, f"partial restore R={R}", 170)
    assert_not_vacuous(co, kw)
    se = e.read_state()
    assert_same_state(se, o.read_state(), R, "partial restore")
    assert_same_logs(se, e.read_log(), o.read_log(), R, "partial restore")
    assert e.digest() == o.digest() and e.step_index == o.step_index == 300
    e.close()
    d.close()


@pytest.mark.parametrize("window", [0, 64], ids=["flat", "ring"])
def test_write_log_alone_rebuilds_the_tail_cache(window):
    """raft_engine_write_log with no write_state before it, on an engine whose
    log-tail cache (the last entry's term and command, the term before it) is
    valid from 170 steps: every command is replaced (the payload only, which
    the protocol never branches on), on the engine and on the oracle.  The
    next appends replicate the new commands, not the cached ones."""
    kw = stress(5, log_window=window)
    n2 = (RING_STEPS if window else STEPS) - 170
    e, o = make_engine(kw, "auto"), O.Oracle(abi.make_params(**kw))
    e.step(170)
    o.step(170, nthreads=NTHREADS)
    d0 = e.digest()
    assert d0 == o.digest()
    lt, lc = e.read_log()
    lc = lc ^ np.uint32(0x5A5A5A5A)
    for x in (e, o):
        x.write_log(lt, lc)
    assert e.digest() == o.digest() != d0
    ce = e.step(n2)
    co = o.step(n2, nthreads=NTHREADS)[:, : abi.NUM_COUNTERS]
    same_counters(ce, co, "write_log alone", 170)
    assert co[:, C["commits"]].sum() > 0 and co[:, C["entries_acked"]].sum() > 0
    assert co[:, C["log_window_miss"]].sum() == 0
    se = e.read_state()
    assert_same_state(se, o.read_state(), 5, "write_log alone")
    assert_same_logs(se, e.read_log(), o.read_log(), 5, "write_log alone")
    assert e.digest() == o.digest()
    e.close()


# ---- e. timer constants ---------------------------------------------------------------

@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", sorted(TIMER_SETS))
@pytest.mark.parametrize("R", [3, 5, 7])
def test_timer_constants(oracle_run, name, R, variant):
    """heartbeat, election and backoff ranges, round timeout and retry, none
    at its default: scale_range over ranges of 2 and of 60,000 values, timers
    that are no multiple of the heartbeat, a round that times out before the
    first tick and a retry that outlasts the round."""
    kw = stress(R, **TIMER_SETS[name])
    check_variant(kw, variant, oracle_run(kw), f"timers {name} R={R} {variant}")


@pytest.mark.parametrize("name", sorted(TIMER_SETS))
def test_timer_constants_textbook(oracle_run, name):
    kw = stress(5, mode=abi.MODE_TEXTBOOK, **TIMER_SETS[name])
    check_variant(kw, "auto", oracle_run(kw), f"textbook timers {name}")


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("R", [3, 5, 7])
def test_degenerate_timer_constants(oracle_run, R, variant):
    """No backoff, a round that times out at once and an immediate retry
    (reference mode): raft_engine_create accepts it and the oracle runs it."""
    kw = stress(R, **DEGENERATE_TIMERS)
    check_variant(kw, variant, oracle_run(kw), f"degenerate timers R={R} {variant}")


# ---- f. the ends of the fault rates ----------------------------------------------------

@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", list(FAULT_EDGES))
def test_fault_rate_edges(oracle_run, name, variant):
    """drop thresholds 1, 1, 2 and 65,536 (every message lost: nobody is ever
    elected), churn threshold 2^32, and partitions that never end, outlast
    their period or are redrawn every step."""
    kw = stress(5, **FAULT_EDGES[name])
    run = oracle_run(kw, vacuous_ok=name == "dropall")
    if name == "dropall":
        assert run.counters[:, C["leaders_elected"]].sum() == 0 and run.counters[:, C["commits"]].sum() == 0
        assert run.counters[:, C["msg_dropped"]].sum() > 0
    if variant == "auto":
        assert expected_net(kw) == abi.step_net_of(kw)
    check_variant(kw, variant, run, f"faults {name} {variant}")


def test_drop_threshold_rounds_up():
    """drop_thr16 = ceil(ppm * 2^16 / 10^6), the oracle's hit16 (u16 * 10^6 <
    ppm * 2^16): 1 ppm and 15 ppm are the same run (threshold 1), 16 ppm is
    another (threshold 2) -- and 1 ppm is not no drops at all."""
    got = {}
    for ppm in (0, 1, 15, 16):
        kw = stress(5, drop_ppm=ppm)
        e = make_engine(kw, "auto")
        c = e.step(STEPS)
        assert e.kernel_info()["net"] == abi.step_net_of(kw)
        got[ppm] = (e.digest(), c.tobytes())
        e.close()
    assert got[1] == got[15]
    assert got[15] != got[16] and got[0] != got[1]
