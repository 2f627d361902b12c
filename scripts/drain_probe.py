"""Time the committed-entry drain (raft_engine_drain_committed_dev) at the bench
size: config 3 at 10^6 x 5 on a flat log, everything committed since step 0
drained after DRAIN_STEPS steps (default "20,400": almost every replica has 0
or 1 new entries, then runs of ~100).

Discipline: one rehearsal drain per point (it allocates the staging), then
lastApplied is zeroed and DRAIN_REPS drains are timed -- each pass between
events on the engine stream (raft_internal_drain_timing: count, scan, expand;
the host's read of the totals between scan and expand is not in them) and the
whole call on the host clock.  Medians are reported.  The byte bound is 24 B
written and 8 B of log read per record plus the 16 B of state words read per
replica, at HBM's 8 TB/s.  Prints one JSON line per point."""
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
G = int(os.environ.get("DRAIN_G", "1000000"))
REPS = int(os.environ.get("DRAIN_REPS", "5"))
STEPS = [int(s) for s in os.environ.get("DRAIN_STEPS", "20,400").split(",")]
CAP = int(os.environ.get("DRAIN_LOG_CAP", "300"))
HBM_BYTES_PER_S = 8e12


def main():
    kw = dict(abi.CONFIGS[3], G=G)
    R = kw["R"]
    lib = abi.load_library()
    lib.raft_internal_drain_timing.argtypes = [C.c_void_p, C.c_int]
    lib.raft_internal_drain_pass_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    e = RaftEngine(abi.make_params(log_cap=CAP, steps_per_launch=abi.BENCH_STEPS_PER_LAUNCH, **kw))
    assert lib.raft_internal_drain_timing(e._h, 1) == abi.RAFT_OK
    zero = np.zeros((G, R), np.int32)
    dev = torch.device("cuda", 0)
    done = 0
    for steps in STEPS:
        e.step(steps - done, counters=False)
        done = steps
        e.set_applied(zero)
        peek = e.peek_committed()
        total = peek["pending"]
        buf = torch.empty(max(total, 1) * 24, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        info = e.drain_committed_dev(buf.data_ptr(), total)              # rehearsal
        assert info["delivered"] == total and info["pending"] == 0, info
        passes, wall = [], []
        ms = (C.c_double * 3)()
        for _ in range(REPS):
            e.set_applied(zero)
            t0 = time.perf_counter()
            info = e.drain_committed_dev(buf.data_ptr(), total)
            wall.append((time.perf_counter() - t0) * 1e3)
            assert info["delivered"] == total, info
            assert lib.raft_internal_drain_pass_ms(e._h, ms) == abi.RAFT_OK
            passes.append(list(ms))
        med = [statistics.median(p[k] for p in passes) for k in range(3)]
        gpu_ms = sum(med)
        bound_ms = (total * 32 + G * R * 16) / HBM_BYTES_PER_S * 1e3
        print(json.dumps({
            "steps": steps, "groups": G, "replicas": R, "log_cap": CAP, "records": total, "reps": REPS,
            "count_ms": round(med[0], 4), "scan_ms": round(med[1], 4), "expand_ms": round(med[2], 4),
            "passes_ms": round(gpu_ms, 4), "call_wall_ms": round(statistics.median(wall), 4),
            "records_per_s_passes": round(total / gpu_ms * 1e3), "records_per_s_call": round(total / statistics.median(wall) * 1e3),
            "byte_bound_ms": round(bound_ms, 4), "passes_over_bound": round(gpu_ms / bound_ms, 2),
            "expand_over_bound": round(med[2] / bound_ms, 2),
            "device_bytes": e.device_bytes, "library_src": abi.build_ids()["library_source_id"]}), flush=True)
        del buf
    e.close()


if __name__ == "__main__":
    main()
