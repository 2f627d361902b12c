"""Time WAL replay (raft_wal_replay_dev) at the bench size beside the poll that
produced its records: config 3 at 10^6 x 5 on a flat log, after REPLAY_STEPS
steps (default 40) and again REPLAY_MORE steps later (default 7).

Each figure is the median of REPLAY_REPS whole calls on the host clock after
one untimed rehearsal (it allocates the staging); every call returns when its
kernels have finished, and the host's read of the totals between the validate
and the apply pass is inside.
  (a) poll_first / replay_first    raft_wal_poll_dev from fresh cursors, and
      raft_wal_replay_dev of those records into a fresh twin (keep_volatile
      off; before every repetition the twin's replicas are put back by an
      amnesia restart of every replica, untimed, so each repetition replays
      onto empty logs as the first did)
      poll_steady / replay_steady  the same REPLAY_MORE steps after a complete
      poll; before every repetition the twin takes the inverse batch (a
      TRUNCATE of every replica back to its length after the first poll, or
      to its length now where that is shorter), untimed
  (b) per record: replay ns / poll ns, and each call's byte bound at 8 TB/s --
      replay: 24 B read, one 32-B sector written per record, four 16-B quads
      read and written per touched replica; poll: 8 B read and 24 B written per
      record, three quads and a 24-B cursor read per replica
  (c) recover_on_device of one replica in each of REPLAY_RECOVER groups
      (default 1000) against the host recover loop over the same replicas,
      both after an amnesia restart of them, on an engine of
      REPLAY_RECOVER_G groups (default 2000): the host image of every node's
      disk (WalImage) is 12 GB of numpy at 10^6 x 5 x 300 slots, filled by a
      Python loop over every record, and
      the host loop's engine-wide cache rebuild per write_state is 500 times
      cheaper there than at the bench size -- the ratio is a lower bound
Prints one JSON line per measurement."""
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

abi = importlib.import_module("raft-kotlin_amd.abi")
RaftEngine = importlib.import_module("raft-kotlin_amd.engine").RaftEngine
RaftService = importlib.import_module("raft-kotlin_amd.service").RaftService
rpl = importlib.import_module("raft-kotlin_amd.replay")
G = int(os.environ.get("REPLAY_G", "1000000"))
REPS = int(os.environ.get("REPLAY_REPS", "5"))
STEPS = int(os.environ.get("REPLAY_STEPS", "40"))
MORE = int(os.environ.get("REPLAY_MORE", "7"))
CAP = int(os.environ.get("REPLAY_LOG_CAP", "300"))
RECOVER = int(os.environ.get("REPLAY_RECOVER", "1000"))
RECOVER_G = int(os.environ.get("REPLAY_RECOVER_G", "2000"))
HBM = 8e12


def timed(call, before, reps):
    """Median wall ms of `call()` over reps, `before()` run untimed ahead of each; one rehearsal first."""
    before()
    info = call()
    ms = []
    for _ in range(reps):
        before()
        t0 = time.perf_counter()
        info = call()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms), ms, info


def main():
    kw = dict(abi.CONFIGS[3], G=G)
    R = kw["R"]
    params = lambda: abi.make_params(log_cap=CAP, steps_per_launch=abi.BENCH_STEPS_PER_LAUNCH, **kw)   # noqa: E731
    a, b = RaftEngine(params()), RaftEngine(params())
    wal = a.wal()
    dev = torch.device("cuda", 0)
    src = abi.build_ids()["library_source_id"]
    rows = {}

    def point(name, records, replicas, med, ms, bound_bytes, info, against=None):
        row = {"what": name, "groups": G, "replicas": R, "log_cap": CAP, "records": records, "touched": replicas,
               "ms": round(med, 4), "reps_ms": [round(x, 4) for x in ms],
               "ns_per_record": round(med * 1e6 / max(records, 1), 3), "bound_ms": round(bound_bytes / HBM * 1e3, 4),
               "vs_bound": round(med / (bound_bytes / HBM * 1e3), 2),
               **{k: info[k] for k in info if k not in ("status", "replicas")}, "library_src": src}
        if against:
            row["vs_poll_per_record"] = round(row["ns_per_record"] / rows[against]["ns_per_record"], 3)
            row["against"] = against
        rows[name] = row
        print(json.dumps(row), flush=True)

    def poll_and_replay(tag, cursors, before_replay):
        wal.set_cursors(cursors)
        total = wal.peek()["pending"]
        buf = torch.empty(max(total, 1) * 24, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        med, ms, info = timed(lambda: wal.poll_dev(buf.data_ptr(), total), lambda: wal.set_cursors(cursors), REPS)
        assert info["delivered"] == total and info["pending"] == 0, info
        b.step_index = a.step_index
        rmed, rms, rinfo = timed(lambda: rpl.replay_dev(b, buf.data_ptr(), total), before_replay, REPS)
        assert rinfo["applied"] == total, rinfo
        touched = rinfo["replicas"]
        point(f"poll_{tag}", total, touched, med, ms, total * 32 + G * R * (3 * 16 + 24), info)
        point(f"replay_{tag}", total, touched, rmed, rms, total * 24 + rinfo["entries"] * 32 + touched * 4 * 32, rinfo,
              f"poll_{tag}")
        return buf, total

    everyone = np.full(G, 0xFF, dtype=np.uint8)
    a.step(STEPS, counters=False)
    fresh = wal.cursors()
    poll_and_replay("first", fresh, lambda: b.restart(everyone, amnesia=True))
    cursors1 = wal.cursors()
    last1 = b.read_state()[:, abi.F_INDEX["last"]:R * abi.NUM_FIELDS:abi.NUM_FIELDS].copy()     # [G, R]
    a.step(MORE, counters=False)
    # the inverse of the steady batch on the twin: every replica cut back to its length after the first poll
    undo = np.zeros(G * R, dtype=abi.WAL_RECORD_DTYPE)
    undo["group"], undo["replica"] = np.repeat(np.arange(G), R), np.tile(np.arange(R), G)
    undo["kind"] = abi.WAL_TRUNCATE
    state = {"calls": 0, "dev": None}

    def before_steady():
        state["calls"] += 1
        if state["calls"] == 1:                      # the rehearsal replays onto the twin as the first poll left it
            return
        if state["dev"] is None:                     # built once, after the rehearsal
            now = b.read_state()[:, abi.F_INDEX["last"]:R * abi.NUM_FIELDS:abi.NUM_FIELDS]
            undo["index"] = np.minimum(last1, now).reshape(-1)
            state["dev"] = torch.from_numpy(undo.view(np.uint8)).to(dev)
            torch.cuda.synchronize(dev)
        rpl.replay_dev(b, state["dev"].data_ptr(), len(undo))

    poll_and_replay("steady", cursors1, before_steady)

    # (c) one replica in each of RECOVER groups: the device call against the host loop
    c = RaftEngine(abi.make_params(log_cap=CAP, **dict(kw, G=RECOVER_G)))
    c.step(STEPS + MORE, counters=False)
    svc = RaftService(c)
    svc.persist()
    nodes = [(int(g), int(g) % R) for g in np.linspace(0, RECOVER_G - 1, RECOVER).astype(np.int64)]
    mask = np.zeros(RECOVER_G, dtype=np.uint8)
    for g, r in nodes:
        mask[g] = 1 << r
    forget = lambda: c.restart(mask, amnesia=True)                                             # noqa: E731
    med, ms, info = timed(lambda: svc.recover_on_device(nodes), forget, REPS)
    hmed, hms, _ = timed(lambda: [svc.recover(g, r) for g, r in nodes], forget, max(1, REPS // 2))
    print(json.dumps({"what": "recover_on_device", "groups": RECOVER_G, "nodes": len(nodes), "ms": round(med, 3),
                      "reps_ms": [round(x, 3) for x in ms], **info, "host_recover_loop_ms": round(hmed, 1),
                      "host_reps_ms": [round(x, 1) for x in hms], "speedup": round(hmed / med, 1),
                      "library_src": src}), flush=True)
    svc.wal.close()
    wal.close()
    for e in (a, b, c):
        e.close()


if __name__ == "__main__":
    main()
