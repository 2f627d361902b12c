"""Time the leader watch (raft_engine_poll_leaders) at the bench size against
the call it replaces, raft_engine_read_leaders over the same range in the same
run: 10^6 x 5 under config 4's fault mix (abi.CONFIGS[3]: drops, isolation
churn, commands), flat log, with timers under which nearly every group has a
leader by step 40.  Three states of the watch:
  all      WATCH_STEPS steps (default 40) from a reset, nothing reported yet:
           every group with a leader is an event.  Before each repetition the
           engine is reset and stepped again, untimed
  none     polled again at once: nothing changed, no event
  deltas   after WATCH_MORE further steps (default 20) of the fault mix: the
           groups whose leader or term changed.  Each repetition steps again,
           untimed, so each sees another 20 steps' worth of changes
In each state the host form (records into a pageable numpy array with room for
every group, as read_leaders' 16 bytes per group go into one), read_leaders,
and the _dev form (records into a device buffer) against its byte bound at
HBM's 8 TB/s: per group the R quad-0 words (16 B each, contiguous) and the 8
bytes of its `seen` pair; per wave of 64 groups that writes, those again; per
event its 24-byte record and its 8-byte pair; 4 + 8 bytes per wave of counts
and offsets when anything is written.

Discipline: one untimed rehearsal per call (it allocates the staging), then
WATCH_REPS timed calls, each between events on the engine stream; medians.
Prints one JSON line per measurement and writes them to WATCH_OUT (default
profiles/watch_probe/watch_probe.jsonl)."""
import ctypes as C
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

abi = importlib.import_module("raft-kotlin_amd.abi")
RaftEngine = importlib.import_module("raft-kotlin_amd.engine").RaftEngine
G = int(os.environ.get("WATCH_G", "1000000"))
REPS = int(os.environ.get("WATCH_REPS", "7"))
STEPS = int(os.environ.get("WATCH_STEPS", "40"))
MORE = int(os.environ.get("WATCH_MORE", "20"))
CAP = int(os.environ.get("WATCH_LOG_CAP", "64"))
OUT = os.environ.get("WATCH_OUT", os.path.join(ROOT, "profiles", "watch_probe", "watch_probe.jsonl"))
HBM_BYTES_PER_S = 8e12
# timers under which a group has a leader within 13 steps (the reference's 20-23 s timeouts over a 2 s
# heartbeat leave a third of the groups in split votes for hundreds of steps)
TIMERS = dict(heartbeat_ms=1500, election_min_ms=7000, election_max_ms=9500, backoff_min_ms=1000,
              backoff_max_ms=4000, round_timeout_ms=11000, retry_ms=3500)


def timed(stream, fn, reps, before=None):
    """Median ms of fn() between events on `stream`, after one rehearsal;
    before() runs untimed ahead of every fn()."""
    out = []
    for k in range(reps + 1):
        if before:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        if k:
            out.append(a.elapsed_time(b))
    return statistics.median(out), out


def main():
    kw = dict(abi.CONFIGS[3], G=G)
    R = kw["R"]
    dev = torch.device("cuda", 0)
    e = RaftEngine(abi.make_params(log_cap=CAP, steps_per_launch=max(STEPS, MORE), **kw, **TIMERS))
    stream = torch.cuda.ExternalStream(e.stream, device=dev)
    lib, h = e._lib, e._h
    host_ev = np.zeros(G, dtype=abi.EVENT_DTYPE)
    host_ld = np.zeros(G, dtype=abi.LEADER_DTYPE)
    dev_ev = torch.zeros(G * 6, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    wi = abi.raft_watch_info()
    base = {"groups": G, "replicas": R, "log_cap": CAP, "steps": STEPS, "more_steps": MORE, "reps": REPS,
            "library_source_id": abi.build_ids()["library_source_id"]}
    lines = []

    def poll_host():
        e._check(lib.raft_engine_poll_leaders(h, 0, G, C.c_void_p(host_ev.ctypes.data), G, C.byref(wi)), "poll_leaders")

    def poll_dev():
        e._check(lib.raft_engine_poll_leaders_dev(h, 0, G, C.c_void_p(dev_ev.data_ptr()), G, C.byref(wi)),
                 "poll_leaders_dev")

    def read_leaders():
        e._check(lib.raft_engine_read_leaders(h, 0, G, C.c_void_p(host_ld.ctypes.data)), "read_leaders")

    def from_reset():
        e.reset()
        e.step(STEPS, counters=False)
        e.sync()

    def step_on():
        e.step(MORE, counters=False)
        e.sync()

    def dev_bytes(events):
        waves = -(-G // 64)
        writing = min(waves, events)                                 # at most: every event in a wave of its own
        return G * (R * 16 + 8) + (writing * 64 * (R * 16 + 8) + events * 32 + waves * 12 if events else 0)

    def emit(name, med, all_ms, **more):
        lines.append(json.dumps({"what": name, **base, "median_ms": round(med, 4),
                                 "all_ms": [round(x, 4) for x in all_ms], **more}))
        print(lines[-1], flush=True)

    def state(name, before_poll):
        """The three calls in one state of the watch.  before_poll puts the state
        (and the watch) where the poll finds it; read_leaders stores nothing, so
        it runs in the state the last poll left."""
        events = []
        med, all_ms = timed(stream, lambda: (poll_host(), events.append(int(wi.delivered))), REPS, before=before_poll)
        ev = int(statistics.median(events[1:]))
        info = {k: int(getattr(wi, k)) for k in abi.WATCH_INFO_FIELDS}
        rl, all_rl = timed(stream, read_leaders, REPS)
        emit(f"read_leaders ({name})", rl, all_rl, bytes_to_host=G * 16)
        emit(f"poll_leaders host ({name})", med, all_ms, events=ev, last_info=info, bytes_to_host=ev * 24 + 4096,
             over_read_leaders=round(med / rl, 3))
        events.clear()
        dmed, all_d = timed(stream, lambda: (poll_dev(), events.append(int(wi.delivered))), REPS,
                            before=before_poll)
        dev_n = int(statistics.median(events[1:]))
        bound = dev_bytes(dev_n) / HBM_BYTES_PER_S * 1e3
        emit(f"poll_leaders_dev ({name})", dmed, all_d, events=dev_n, mix_bytes_per_group=round(dev_bytes(dev_n) / G, 1),
             mix_bound_ms=round(bound, 4), over_mix_bound=round(dmed / bound, 2), over_read_leaders=round(dmed / rl, 3))
        return med, rl

    state("all", from_reset)
    none_ms, none_rl = state("none", None)
    state("deltas", step_on)
    verdict = {"what": "expectation", **base, "poll_none_ms": round(none_ms, 4), "read_leaders_ms": round(none_rl, 4),
               "poll_with_no_event_beats_read_leaders": bool(none_ms < none_rl)}
    lines.append(json.dumps(verdict))
    print(lines[-1], flush=True)
    e.close()
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
