"""Time the state machine's apply (raft_engine_sm_apply) against the drain
(raft_engine_drain_committed_dev) over the same entries: config 3 at 10^6 x 5 on
a flat log, everything committed since step 0 consumed after SM_STEPS steps
(default "20,400": almost every replica has 0 or 1 new entries, then runs of
~100), with SM_SLOTS registers per replica (default "8").

Discipline: both cursors are zeroed before every call, so every call consumes
the same entries; one untimed rehearsal of each (it allocates the staging), then
SM_REPS timed calls of each, alternating.  Each call sits between two events on
the engine stream (for the drain that span holds the host's read of the scan's
total between its passes: it is part of what the call costs), and on the host
clock; the apply kernel alone is timed by the library's own events
(raft_internal_sm_timing), the drain's passes by raft_internal_drain_timing.
Medians are reported.  Prints one JSON line per point."""
import ctypes as C
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
G = int(os.environ.get("SM_G", "1000000"))
REPS = int(os.environ.get("SM_REPS", "5"))
STEPS = [int(s) for s in os.environ.get("SM_STEPS", "20,400").split(",")]
SLOTS = [int(s) for s in os.environ.get("SM_SLOTS", "8").split(",")]
CAP = int(os.environ.get("SM_LOG_CAP", "300"))


def main():
    kw = dict(abi.CONFIGS[3], G=G)
    R = kw["R"]
    lib = abi.load_library()
    lib.raft_internal_drain_timing.argtypes = [C.c_void_p, C.c_int]
    lib.raft_internal_drain_pass_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    lib.raft_internal_sm_timing.argtypes = [C.c_void_p, C.c_int]
    lib.raft_internal_sm_kernel_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    e = RaftEngine(abi.make_params(log_cap=CAP, steps_per_launch=abi.BENCH_STEPS_PER_LAUNCH, **kw))
    assert lib.raft_internal_drain_timing(e._h, 1) == abi.RAFT_OK
    assert lib.raft_internal_sm_timing(e._h, 1) == abi.RAFT_OK
    zero = np.zeros((G, R), np.int32)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.ExternalStream(e.stream, device=dev)

    def timed(call):
        """(result, ms between events on the engine stream, host ms)"""
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        t0 = time.perf_counter()
        res = call()
        wall = (time.perf_counter() - t0) * 1e3
        b.record(stream)
        b.synchronize()
        return res, a.elapsed_time(b), wall

    done = 0
    for steps in STEPS:
        e.step(steps - done, counters=False)
        done = steps
        e.set_applied(zero)
        total = e.peek_committed()["pending"]
        buf = torch.empty(max(total, 1) * 24, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        for S in SLOTS:
            e.sm_configure(S)
            e.set_applied(zero)
            assert e.sm_apply()["applied"] == total                          # rehearsals
            assert e.drain_committed_dev(buf.data_ptr(), total)["delivered"] == total
            ap_ev, ap_wall, ap_kern, dr_ev, dr_wall, dr_pass = [], [], [], [], [], []
            ms, ps = C.c_double(), (C.c_double * 3)()
            for _ in range(REPS):
                e.sm_configure(S)                                            # zeroes the machine: the same entries again
                info, ev, wall = timed(e.sm_apply)
                assert info["applied"] == total and info["regressed"] == 0, info
                assert lib.raft_internal_sm_kernel_ms(e._h, C.byref(ms)) == abi.RAFT_OK
                ap_ev.append(ev), ap_wall.append(wall), ap_kern.append(ms.value)
                e.set_applied(zero)
                info, ev, wall = timed(lambda: e.drain_committed_dev(buf.data_ptr(), total))
                assert info["delivered"] == total, info
                assert lib.raft_internal_drain_pass_ms(e._h, ps) == abi.RAFT_OK
                dr_ev.append(ev), dr_wall.append(wall), dr_pass.append(sum(ps))
            med = statistics.median
            print(json.dumps({
                "steps": steps, "groups": G, "replicas": R, "log_cap": CAP, "slots": S, "entries": total, "reps": REPS,
                "config": 3, "seed": kw["seed"], "drop_ppm": kw["drop_ppm"], "churn_ppm": kw["churn_ppm"],
                "churn_steps": kw["churn_steps"], "cmd_ppm": kw["cmd_ppm"],
                "apply_kernel_ms": round(med(ap_kern), 4), "apply_call_event_ms": round(med(ap_ev), 4),
                "apply_call_wall_ms": round(med(ap_wall), 4),
                "drain_passes_ms": round(med(dr_pass), 4), "drain_call_event_ms": round(med(dr_ev), 4),
                "drain_call_wall_ms": round(med(dr_wall), 4),
                "apply_entries_per_s": round(total / med(ap_ev) * 1e3), "drain_entries_per_s": round(total / med(dr_ev) * 1e3),
                "apply_kernel_entries_per_s": round(total / med(ap_kern) * 1e3),
                "apply_over_drain": round(med(ap_ev) / med(dr_ev), 3),
                "device_bytes": e.device_bytes, "library_src": abi.build_ids()["library_source_id"]}), flush=True)
        del buf
    e.close()


if __name__ == "__main__":
    main()
