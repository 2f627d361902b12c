"""The log-tail cache after every device-side writer (marker `gpu`).

Every replica carries three words no accessor exports: t1, t2 (the terms of
log[last - 1] and log[last - 2]) and c1 (the command of log[last - 1]).  The
step kernel, the handler batches, the routed proposals, leadership transfer and
the no-op entries read them from HBM instead of the log; eight kinds of device
code write them.  A host write marks them stale and the next consumer rebuilds
them -- which is why a wrong word a device writer leaves is invisible to
read_state and to every test that starts from write_state / write_log.

Here the words are read back (raft-kotlin_amd/debug.py) after every call that
writes them, and held to what the engine's own state and logs define
(tail_cache_model.derive, rebuild_cache_kernel's rule), exactly, on every word
whose slot is retained.  The call sequences are tail_cache_model.SCENARIOS: each
was recorded on the oracle (tests/test_tail_cache_cpu.py asserts its conditions
there) and is played here call by call, the results compared with the oracle's.

Which scenario pins which writer:
  log_add in the step kernel            step-*  (ghost tails, overwrites, truncations, rings, every kernel)
  log_add / store_rep in the batches    handlers-*, consumer-*  (both batch paths)
  the propose kernel                    client-propose-*  (ghost tails, LOG_FULL)
  the no-op kernel                      client-noops-*
  the outbox pump's re-propose          outbox-*
  restart_kernel                        restart-*  (mask and random form; amnesia zeroes the words)
  install_kernel                        install-*  (flat, and a ring with the leader's floor above 0)
  replay_apply                          replay-*  (whole, pieces, TRUNCATE keep 0 / 1 / 2, lone HARDSTATE, ...)
"""
import importlib

import numpy as np
import pytest

import tail_cache_model as TC
from helpers import abi, assert_same_logs, assert_same_state

pytestmark = pytest.mark.gpu

RaftEngine = importlib.import_module("raft-kotlin_amd.engine").RaftEngine
dbg = importlib.import_module("raft-kotlin_amd.debug")
rpl = importlib.import_module("raft-kotlin_amd.replay")

assert_cache = TC.assert_cache


def engine_of(sc):
    e = RaftEngine(abi.make_params(**sc["kw"]))
    if sc.get("slots"):
        e.sm_configure(sc["slots"])
    return e


def play(name, path=None):
    """Scenario `name` on an engine: the oracle's recorded calls, assert_cache
    after every writer, and at the end the oracle's state, logs and digest."""
    sc, run = TC.SCENARIOS[name], TC.host_run(name)
    with engine_of(sc) as e:
        if path is not None:
            e.set_batch_path(path)
        cache, valid = dbg.read_tail_cache(e)
        assert valid == 1 and not cache.any(), f"{name}: a fresh engine"
        if TC.play(e, run["trace"], assert_cache, name):              # no access below a window: parity to the end
            se = e.read_state()
            assert_same_state(se, run["state"], e.R, name)
            assert_same_logs(se, e.read_log(), run["logs"], e.R, name)
            assert e.digest() == run["digest"], name


PATHS = {"bucketed": abi.BATCH_PATH_BUCKETED, "sorted": abi.BATCH_PATH_SORTED}
BATCH = [n for n, sc in TC.SCENARIOS.items() if sc.get("paths")]
OTHER = [n for n, sc in TC.SCENARIOS.items() if not sc.get("paths")]


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("name", BATCH)
def test_cache_after_the_handler_batches(name, path):
    """append_batch and append_command_batch (log_add, store_rep) on both batch
    paths, and the consumer sequence: what they stored back is read by a vote
    batch, by an append batch whose prev sits on t1 / t2, and by 20 steps."""
    play(name, PATHS[path])


@pytest.mark.parametrize("name", OTHER)
def test_cache_after_every_other_writer(name):
    """The step kernels, the client writers, restart, install and replay."""
    play(name)


# ---- the validity protocol
KW = dict(R=5, G=203, seed=11, log_cap=64, cmd_ppm=500_000, drop_ppm=50_000)


def stale(e, label):
    cache, valid = dbg.read_tail_cache(e)
    assert valid == 0, f"{label}: the cache is marked current"
    again, valid = dbg.read_tail_cache(e)
    assert valid == 0 and np.array_equal(cache, again), f"{label}: reading changed something"


def test_fresh_and_reset_engines():
    with RaftEngine(abi.make_params(**KW)) as e:
        for what in ("fresh", "reset"):
            cache, valid = dbg.read_tail_cache(e)
            assert valid == 1 and cache.shape == (203, 5, 3) and not cache.any(), what
            part, valid = dbg.read_tail_cache(e, 200, 3)
            assert valid == 1 and part.shape == (3, 5, 3)
            assert dbg.read_tail_cache(e, 203, 0)[0].shape == (0, 5, 3)
            e.step(30)
            state, cache = assert_cache(e, what)
            assert cache.any()
            assert np.array_equal(dbg.read_tail_cache(e, 7, 100)[0], cache[7:107])   # a range is the same words
            e.reset()
        with pytest.raises(importlib.import_module("raft-kotlin_amd.engine").RaftError):
            dbg.read_tail_cache(e, 200, 4)                          # a range outside the engine


def loaded(e):
    """An image 40 steps produce, read back."""
    e.step(40)
    return e.read_state(), e.read_log()


def test_host_writes_mark_the_cache_stale_and_the_accessor_leaves_it():
    with RaftEngine(abi.make_params(**KW)) as e:
        st, (t, c) = loaded(e)
        digest = e.digest()
        e.write_state(st)
        stale(e, "write_state alone")
        e.step(1)
        assert_cache(e, "a step after write_state")
        st, (t, c) = e.read_state(), e.read_log()
        e.write_log(t, c)
        stale(e, "write_log alone")
        e.step(1)
        assert_cache(e, "a step after write_log")
        e.write_state(e.read_state(3, 10), 3)
        stale(e, "a partial-range write")
        e.step(1)
        assert_cache(e, "a step after a partial write")
        assert digest != e.digest()


CONSUMERS = ["step", "vote_batch", "append_batch", "append_command_batch", "propose", "transfer", "append_noops"]


@pytest.mark.parametrize("consumer", CONSUMERS)
def test_every_consumer_rebuilds_a_stale_cache(consumer):
    with RaftEngine(abi.make_params(**KW)) as e:
        st, (t, c) = loaded(e)
        e.write_state(st)
        e.write_log(t, c)
        stale(e, "loaded")
        rng = np.random.default_rng(3)
        grp, dst = rng.integers(0, e.G, 300), rng.integers(0, e.R, 300).astype(np.int32)
        if consumer == "step":
            e.step(1)
        elif consumer == "vote_batch":
            e.vote_batch(grp, dst, np.stack([rng.integers(0, 6, 300), rng.integers(1, 6, 300), rng.integers(0, 9, 300),
                                             rng.integers(0, 4, 300)], 1).astype(np.int32))
        elif consumer == "append_batch":
            e.append_batch(*TC.tail_appends(rng, st, t, 300, e.R))
        elif consumer == "append_command_batch":
            e.append_command_batch(grp, dst, rng.integers(0, 1 << 32, 300, dtype=np.uint64).astype(np.uint32))
        elif consumer == "propose":
            e.propose(np.arange(e.G, dtype=np.int64), np.arange(e.G, dtype=np.uint32))
        elif consumer == "transfer":
            e.transfer(np.arange(e.G, dtype=np.int64))
        else:
            e.append_noops(cmd=0xFFFF0001)
        assert_cache(e, f"after {consumer}")


@pytest.mark.parametrize("writer", ["restart", "install_snapshot", "replay"])
def test_writers_that_rebuild_nothing_leave_the_cache_stale(writer):
    """restart, install_snapshot and replay keep a current cache current but do
    not rebuild a stale one: the flag stays 0, and one step later the words are
    the log's."""
    with RaftEngine(abi.make_params(**KW)) as e:
        e.sm_configure(4)
        st, (t, c) = loaded(e)
        e.sm_apply()
        e.write_state(st)
        e.write_log(t, c)
        if writer == "restart":
            assert e.restart(ppm=300_000)["restarted"] > 0
        elif writer == "install_snapshot":
            e.install_snapshot()
        else:
            import wal_model as WM
            rows = [(g, 1, WM.HS, -1, 9, 0, -1) for g in range(0, e.G, 2)]
            assert rpl.replay(e, WM.records(rows))["replicas"] == len(rows)
        stale(e, f"a host write, then {writer}")
        e.step(1)
        assert_cache(e, f"one step after {writer}")
