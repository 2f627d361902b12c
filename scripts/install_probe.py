"""Time a snapshot install on the device (raft_engine_install_snapshot) against
the byte bound of the words it must move and against the copies of the host
route that did the same before it existed (read_state + read_log + sm_read,
write_state + write_log + sm_write): config 3 at 10^6 x 5 with an 8-register
machine, on a flat log (INSTALL_LOG_CAP, default 300) and on a ring
(INSTALL_WINDOW, default 16), after INSTALL_STEPS steps (default 40).

Cases, per log form: an AMNESIA restart_random at each INSTALL_PPM rate (default
"1000,100000,1000000") followed by install(min_lag=1), which heals exactly the
replicas the restart emptied in the groups that kept a leader (at 10^6 ppm every
leader is restarted too, so nothing can be installed: the case times the
kernel's read-only pass); and "all": no restart, install(min_lag=0), every
follower of every group with a leader, the largest copy there is.

Discipline: the restart at an unchanged step index selects the same replicas
and the install puts them back level with their leader, so every repetition
does the same work on the same state; the restart is outside the timed region.
One untimed rehearsal, then INSTALL_REPS timed calls; the call ends in a device
synchronise, so it is timed on the host clock, and it sits between two events
on the engine stream.  The host route is timed on groups [0, INSTALL_HOST_G)
only (default 10^5: the logs of 10^6 groups are 12 GB of host memory each way)
and its copies alone, no edit.  Medians are reported.  Prints one JSON line per
case."""
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

abi = importlib.import_module("raft-kotlin_amd.abi")
eng = importlib.import_module("raft-kotlin_amd.engine")
G = int(os.environ.get("INSTALL_G", "1000000"))
HOST_G = min(G, int(os.environ.get("INSTALL_HOST_G", "100000")))
REPS = int(os.environ.get("INSTALL_REPS", "5"))
STEPS = int(os.environ.get("INSTALL_STEPS", "40"))
PPMS = [int(s) for s in os.environ.get("INSTALL_PPM", "1000,100000,1000000").split(",")]
CAP = int(os.environ.get("INSTALL_LOG_CAP", "300"))
WINDOW = int(os.environ.get("INSTALL_WINDOW", "16"))
SLOTS = 8


def moved_bytes(info: dict) -> int:
    """Both directions: per installed replica 4 state quads, the head and the
    registers read (the leader's or its own) and written; per slot 8 bytes each way."""
    return info["installed"] * 2 * (4 * 16 + 16 + SLOTS * 4) + info["slots_copied"] * 2 * 8


def timed_install(e, stream, min_lag):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    t0 = time.perf_counter()
    info = e.install_snapshot(min_lag=min_lag)
    wall = (time.perf_counter() - t0) * 1e3
    b.record(stream)
    b.synchronize()
    return info, wall, a.elapsed_time(b)


def host_copies(e):
    t0 = time.perf_counter()
    st = e.read_state(0, HOST_G)
    t, c = e.read_log(0, HOST_G)
    h, r = e.sm_read(0, HOST_G)
    t1 = time.perf_counter()
    e.write_state(st, 0)
    e.write_log(t, c, 0)
    e.sm_write(h, r, 0)
    e.sync()
    t2 = time.perf_counter()
    return (t1 - t0) * 1e3, (t2 - t1) * 1e3, st.nbytes + t.nbytes + c.nbytes + h.nbytes + r.nbytes


def main():
    med = statistics.median
    for window in (0, WINDOW):
        kw = dict(abi.CONFIGS[3], G=G)
        e = eng.RaftEngine(abi.make_params(log_cap=CAP, log_window=window, steps_per_launch=abi.BENCH_STEPS_PER_LAUNCH, **kw))
        e.sm_configure(SLOTS)
        stream = torch.cuda.ExternalStream(e.stream, device=torch.device("cuda", 0))
        for _ in range(STEPS // 10):                                  # applied often enough that no ring leader is gapped
            e.step(10, counters=False)
            e.sm_apply()
        for case in ["all", *PPMS]:                                  # "all" first: the restarts take leaders away
            min_lag = 0 if case == "all" else 1
            walls, evs, info, same = [], [], None, True
            for rep in range(REPS + 1):                               # rep 0: the untimed rehearsal
                rinfo = e.restart(ppm=case, amnesia=True) if case != "all" else None
                got, wall, ev = timed_install(e, stream, min_lag)
                if rep:
                    same = same and got == info                       # the same work every repetition
                    walls.append(wall)
                    evs.append(ev)
                info = got
            nbytes = moved_bytes(info)
            print(json.dumps({
                "case": case, "log_window": window, "groups": G, "replicas": kw["R"], "log_cap": CAP, "sm_slots": SLOTS,
                "steps": STEPS, "reps": REPS, "config": 3, "seed": kw["seed"], "min_lag": min_lag, "same_work_every_rep": same,
                "restarted": rinfo["restarted"] if rinfo else 0, **info,
                "install_call_wall_ms": round(med(walls), 4), "install_call_event_ms": round(med(evs), 4),
                "moved_bytes": nbytes, "moved_gb_per_s_event": round(nbytes / med(evs) / 1e6, 1) if nbytes else 0.0,
                "library_src": abi.build_ids()["library_source_id"]}), flush=True)
        rd, wr = [], []
        for rep in range(REPS + 1):
            r_ms, w_ms, nb = host_copies(e)
            if rep:
                rd.append(r_ms)
                wr.append(w_ms)
        print(json.dumps({
            "case": "host_route_copies", "log_window": window, "groups": HOST_G, "of_groups": G, "log_cap": CAP,
            "read_ms": round(med(rd), 3), "write_ms": round(med(wr), 3), "bytes_each_way": nb,
            "scaled_to_all_groups_ms": round((med(rd) + med(wr)) * G / HOST_G, 1),
            "library_src": abi.build_ids()["library_source_id"]}), flush=True)
        e.close()


if __name__ == "__main__":
    main()
