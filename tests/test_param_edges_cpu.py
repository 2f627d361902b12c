"""The parameter corners on the two independent CPU implementations: the scalar
oracle (oracle/raft_oracle.c) against the SoA backend (oracle/raft_soa.cpp),
bit-exact, at 64-bit seeds, global group ids with bit 31 set, step indices up
to and across the 32-bit wrap, non-default timer constants and the ends of the
fault rates -- the parameter sets test_gpu_param_edges.py runs on the HIP
engine, where the oracle is the reference.  Reference mode and a flat log: all
the SoA backend models.  Also the oracle's own export / restore, which the
GPU resume tests lean on."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
from helpers import (DEGENERATE_TIMERS, FAULT_EDGES, SEEDS64, STRESS_MIX, TIMER_SETS, abi, assert_not_vacuous,
                     assert_same_logs, assert_same_state, high_g0)

G, STEPS, CAP = 300, 200, 200
LE, CM = abi.C_INDEX["leaders_elected"], abi.C_INDEX["commits"]


def base(R=5, **kw):
    return dict(dict(R=R, G=G, seed=11, log_cap=CAP, **STRESS_MIX), **kw)


def run_both(kw, t0=None, steps=STEPS, vacuous_ok=False):
    """Oracle and SoA side by side: per-step counters, state, logs and digest
    equal; returns the oracle's (counters, digest)."""
    o, s = O.Oracle(abi.make_params(**kw)), O.Soa(abi.make_params(**kw))
    try:
        if t0 is not None:
            o.step_index = t0
            s.set_step_index(t0)
        assert_same_state(o.read_state(), s.read_state(), kw["R"], "init")
        rows = []
        for chunk, threads in ((1, 1), (37, 3), (steps - 38, 16)):
            co, cs = o.step(chunk, nthreads=4), s.step(chunk, nthreads=threads)
            np.testing.assert_array_equal(co, cs)
            assert o.digest() == s.digest()
            rows.append(co)
        so = o.read_state()
        assert_same_state(so, s.read_state(), kw["R"], "final")
        assert_same_logs(so, o.read_log(), s.read_log(), kw["R"], "final")
        co = np.concatenate(rows)[:, : abi.NUM_COUNTERS]
        if not vacuous_ok:
            assert_not_vacuous(co, kw)
        if t0 is not None:
            assert o.step_index == (t0 + steps) % (1 << 32)
        return co, o.digest()
    finally:
        o.close()
        s.close()


def test_make_params_keeps_a_64_bit_seed():
    for s in SEEDS64 + [(1 << 64) - 1]:
        assert abi.make_params(seed=s).seed == s


def test_oracle_philox_key1_matches_the_host_library():
    """oracle/philox_ref.h against the engine's philox.h (its host side) at
    keys whose high word is not 0, which the Random123 vectors barely set."""
    try:
        lib = abi.load_library()
    except (RuntimeError, OSError) as e:
        pytest.skip(f"the engine library does not load here: {e}")
    rng = np.random.default_rng(5)
    keys = [(7, 0x9E3779B9), (0x7F4A7C15, 0x9E3779B9), (0, 1), (0, 0xFFFFFFFF), (0xFFFFFFFF, 0x80000000)]
    keys += [tuple(int(x) for x in rng.integers(0, 1 << 32, 2)) for _ in range(20)]
    for key in keys:
        ctr = [int(x) for x in rng.integers(0, 1 << 32, 4)]
        out = (C.c_uint32 * 4)()
        lib.raft_philox4x32_10((C.c_uint32 * 4)(*ctr), (C.c_uint32 * 2)(*key), out)
        assert list(out) == O.philox(ctr, key), (ctr, key)
        assert list(out) != O.philox(ctr, (key[0], key[1] ^ 1))       # key1 is in the function


@pytest.mark.parametrize("R", [3, 5, 7])
def test_seeds_64_bit(R):
    """The two seeds that share key0 must not share a run."""
    dg = [run_both(base(R, seed=s))[1] for s in SEEDS64]
    assert len(set(dg)) == 3


@pytest.mark.parametrize("R", [3, 5, 7])
@pytest.mark.parametrize("where", ["top", "bit31"])
def test_high_global_ids(R, where):
    g0 = high_g0(G)[where]
    full, dfull = run_both(base(R, g0=g0))
    a, da = run_both(base(R, g0=g0, G=130), vacuous_ok=True)
    b, db = run_both(base(R, g0=g0 + 130, G=G - 130), vacuous_ok=True)
    np.testing.assert_array_equal(full, a + b)
    assert dfull == (da + db) % (1 << 64)
    if where == "top":                                              # bit 31 of the id is in the draws
        assert not np.array_equal(full, run_both(base(R, g0=g0 - (1 << 31)))[0])


@pytest.mark.parametrize("R", [3, 5, 7])
@pytest.mark.parametrize("t0", [(1 << 32) - 1000, (1 << 32) - 150], ids=["high", "wrap"])
def test_high_step_indices(R, t0):
    """Step indices near 2^32 and across it: the counter wraps, the draws and
    the partition phase are taken in uint32_t."""
    c, dg = run_both(base(R), t0=t0)
    assert dg != run_both(base(R), t0=t0 & 0x7FFFFFFF)[1]


@pytest.mark.parametrize("R", [3, 5, 7])
@pytest.mark.parametrize("name", sorted(TIMER_SETS) + ["degenerate"])
def test_timer_constants(R, name):
    run_both(base(R, **(TIMER_SETS[name] if name in TIMER_SETS else DEGENERATE_TIMERS)))


def test_fault_rate_edges():
    runs = {}
    for name, over in FAULT_EDGES.items():
        kw = base(5, **over)
        c, dg = run_both(kw, vacuous_ok=name == "dropall")
        runs[name] = (c.tobytes(), dg)
        if name == "dropall":                                        # nobody hears anybody
            assert c[:, LE].sum() == 0 and c[:, CM].sum() == 0
            assert c[:, abi.C_INDEX["msg_dropped"]].sum() > 0
    # hit16 is u16 * 10^6 < ppm * 2^16: thresholds ceil(ppm * 0.065536) = 1, 1, 2
    assert runs["drop1"] == runs["drop15"] != runs["drop16"]


def restore_kw(case):
    return {"flat": base(5), "ring": base(5, log_window=64), "cmd_limit": base(5, cmd_limit=30),
            "churn": base(5, churn_ppm=200_000), "R7": base(7), "R3-no-faults": dict(R=3, G=G, seed=11, log_cap=CAP,
                                                                                     cmd_ppm=500_000),
            "textbook": base(5, mode=abi.MODE_TEXTBOOK, ae_max_entries=4)}[case]


@pytest.mark.parametrize("case", ["flat", "ring", "cmd_limit", "churn", "R7", "R3-no-faults", "textbook"])
def test_oracle_restore_resumes_bit_exact(case):
    """An oracle run exported at step 170 (read_state, read_log, step_index)
    and restored into a fresh oracle continues exactly as the uninterrupted
    run: the canonical export carries everything a step reads."""
    kw = restore_kw(case)
    a = O.Oracle(abi.make_params(**kw))
    c1 = a.step(170, nthreads=4)[:, : abi.NUM_COUNTERS]
    b = O.Oracle(abi.make_params(**kw))
    st, lg = a.read_state(), a.read_log()
    b.write_state(st)
    b.write_log(*lg)
    b.step_index = a.step_index
    assert b.step_index == 170 and b.digest() == a.digest()
    assert_same_state(b.read_state(), st, kw["R"], case)
    ca, cb = a.step(130, nthreads=4), b.step(130, nthreads=3)
    np.testing.assert_array_equal(ca, cb)
    assert_not_vacuous(np.concatenate([c1, ca[:, : abi.NUM_COUNTERS]]), kw, case)
    sa = a.read_state()
    assert_same_state(sa, b.read_state(), kw["R"], case)
    assert_same_logs(sa, a.read_log(), b.read_log(), kw["R"], case)
    assert a.digest() == b.digest()
    if case == "ring":
        assert int(np.max(sa[:, [r * abi.NUM_FIELDS + abi.F_INDEX["phys"] for r in range(5)]])) > 64
    if case == "churn":
        assert np.any(st[:, -2] != 0)


@pytest.mark.parametrize("R", [3, 5, 7])
def test_oracle_partial_restore(R):
    """Groups [7, 37) of another run (another seed, at its step 170) written
    into a run at step 170: they go on as in their own run, the others as in
    theirs, and read_state / read_log at that offset return what was written."""
    kw, kw2 = base(R), base(R, seed=12)
    a, d = O.Oracle(abi.make_params(**kw)), O.Oracle(abi.make_params(**kw2))
    a.step(170, nthreads=4)
    d.step(170, nthreads=4)
    st, (lt, lc) = d.read_state(7, 30), d.read_log(7, 30)
    a.write_state(st, 7)
    a.write_log(lt, lc, 7)
    assert_same_state(a.read_state(7, 30), st, R, "read back")
    assert_same_logs(st, a.read_log(7, 30), (lt, lc), R, "read back")
    s = O.Soa(abi.make_params(**kw))                     # the same on the SoA backend
    s.step(170, nthreads=4)
    s.write_state(st, 7)
    s.write_log(lt, lc, 7)
    np.testing.assert_array_equal(a.step(130, nthreads=4), s.step(130, nthreads=4))
    h = O.Oracle(abi.make_params(**kw))                  # the host run, never written to
    h.step(300, nthreads=4)
    sa, sh = a.read_state(), h.read_state()
    keep = np.r_[0:7, 37:G]
    assert_same_state(sa[keep], sh[keep], R, "untouched groups")
    assert not np.array_equal(sa[7:37], sh[7:37])
    assert_same_state(sa, s.read_state(), R, "soa")
    assert_same_logs(sa, a.read_log(), s.read_log(), R, "soa")
    assert a.digest() == s.digest()
    for x in (a, d, h, s):
        x.close()
