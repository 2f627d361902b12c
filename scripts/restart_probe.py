"""Time a seeded restart on the device (raft_engine_restart_random) against the
host route that did the same before it existed -- read_state, edit the words,
write_state -- for the same selection: config 3 at 10^6 x 5 on a flat log after
RESTART_STEPS steps (default 40), at RESTART_PPM rates (default
"1000,100000,1000000").

Discipline: a persistent restart (flags 0) of a replica that was just
restarted at the same step index stores the same words again, so every
repetition does the same work on the same state; one untimed rehearsal of each
route (it allocates the staging), then RESTART_REPS timed calls of each,
alternating.  Both routes end in a device synchronise, so each is timed on the
host clock; the device call also sits between two events on the engine stream.
The host route's edit is timed apart: it is numpy on the selection, which a
real caller would also pay, but it is not the engine's cost.  Medians are
reported.  Prints one JSON line per rate."""
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
eng = importlib.import_module("raft-kotlin_amd.engine")
G = int(os.environ.get("RESTART_G", "1000000"))
REPS = int(os.environ.get("RESTART_REPS", "5"))
STEPS = int(os.environ.get("RESTART_STEPS", "40"))
PPMS = [int(s) for s in os.environ.get("RESTART_PPM", "1000,100000,1000000").split(",")]
CAP = int(os.environ.get("RESTART_LOG_CAP", "300"))
NF = abi.NUM_FIELDS


def host_edit(st, before, sel, R):
    """The canonical words of a persistent restart, taken from a device restart's
    result `st` for the election timeouts (the probe times the route, not a
    second Philox): role, commit, timers, flags, the session rows."""
    out = before.copy()
    for r in range(R):
        rows = np.flatnonzero(sel[:, r])
        for f in ("role", "commit", "election_ms", "flags", "phase_ms", "retry_ms"):
            out[rows, r * NF + abi.F_INDEX[f]] = st[rows, r * NF + abi.F_INDEX[f]]
        out[rows, R * NF + r * R:R * NF + (r + 1) * R] = 0
        out[rows, R * NF + R * R + r * R:R * NF + R * R + (r + 1) * R] = 0
    return out


def main():
    kw = dict(abi.CONFIGS[3], G=G)
    R = kw["R"]
    e = eng.RaftEngine(abi.make_params(log_cap=CAP, steps_per_launch=abi.BENCH_STEPS_PER_LAUNCH, **kw))
    dev = torch.device("cuda", 0)
    stream = torch.cuda.ExternalStream(e.stream, device=dev)
    e.step(STEPS, counters=False)
    med = statistics.median
    for ppm in PPMS:
        before = e.read_state()
        info = e.restart(ppm=ppm)                                               # rehearsal of the device route
        after = e.read_state()
        d = before != after
        sel = np.stack([d[:, r * NF:(r + 1) * NF].any(axis=1) for r in range(R)], axis=1)
        e.write_state(host_edit(after, before, sel, R))                         # rehearsal of the host route
        assert np.array_equal(e.read_state(), after)
        dev_wall, dev_ev, host_wall, host_edit_ms = [], [], [], []
        for _ in range(REPS):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            t0 = time.perf_counter()
            again = e.restart(ppm=ppm)
            dev_wall.append((time.perf_counter() - t0) * 1e3)
            b.record(stream)
            b.synchronize()
            dev_ev.append(a.elapsed_time(b))
            assert again["restarted"] == info["restarted"]                       # (its leaders are followers by now)
            t0 = time.perf_counter()
            st = e.read_state()
            t1 = time.perf_counter()
            st = host_edit(after, st, sel, R)
            t2 = time.perf_counter()
            e.write_state(st)
            t3 = time.perf_counter()
            host_wall.append((t1 - t0 + t3 - t2) * 1e3)
            host_edit_ms.append((t2 - t1) * 1e3)
        assert np.array_equal(e.read_state(), after)
        print(json.dumps({
            "ppm": ppm, "groups": G, "replicas": R, "log_cap": CAP, "steps": STEPS, "reps": REPS, "config": 3,
            "seed": kw["seed"], "restarted": info["restarted"], "leaders": info["leaders"],
            "changed_replicas": int(sel.sum()),
            "device_call_wall_ms": round(med(dev_wall), 4), "device_call_event_ms": round(med(dev_ev), 4),
            "host_route_wall_ms": round(med(host_wall), 4), "host_edit_ms": round(med(host_edit_ms), 4),
            "state_bytes_each_way": G * abi.group_words(R) * 4,
            "host_over_device": round(med(host_wall) / med(dev_wall), 1),
            "library_src": abi.build_ids()["library_source_id"]}), flush=True)
    e.close()


if __name__ == "__main__":
    main()
