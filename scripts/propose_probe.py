"""Time the client path (raft_propose_batch_dev, raft_engine_resolve_tickets_dev)
at the bench size: config 3 at 10^6 x 5 on a flat log after PROPOSE_STEPS steps
(default 400), PROPOSE_N (default 10^6) uniformly random proposals from device
buffers.

Yardstick of the propose: the same library's raft_append_command_batch_dev on
the same messages with the replicas precomputed from read_leaders (a group
without a leader: replica 0, so that every message is an append there too).
That path does strictly less -- no routing read, no ticket store -- on its
default (bucketed) ordering; its sorted ordering (a radix sort of every message,
as the propose does) is timed too, so the ratio splits into the ordering's share
and the routing's.  Yardstick of the resolve: its byte bound at HBM's 8 TB/s,
per ticket 28 B in, 16 B out and, per replica, two 32-B state sectors (quad 1:
lastIndex / physLen, quad 2: commitIndex) and one 32-B log sector.

Discipline: one untimed rehearsal per call (it allocates the staging), then
PROPOSE_REPS timed calls, each between events on the engine stream; medians.
Every timed propose / command batch appends to the logs (log_cap leaves room).
Prints one JSON line per measurement."""
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
G = int(os.environ.get("PROPOSE_G", "1000000"))
N = int(os.environ.get("PROPOSE_N", "1000000"))
REPS = int(os.environ.get("PROPOSE_REPS", "5"))
STEPS = int(os.environ.get("PROPOSE_STEPS", "400"))
CAP = int(os.environ.get("PROPOSE_LOG_CAP", "300"))
HBM_BYTES_PER_S = 8e12


def timed(stream, fn, reps):
    """Median ms of fn() between events on `stream`, after one rehearsal."""
    fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out), out


def main():
    kw = dict(abi.CONFIGS[3], G=G)
    R = kw["R"]
    dev = torch.device("cuda", 0)
    e = RaftEngine(abi.make_params(log_cap=CAP, steps_per_launch=abi.BENCH_STEPS_PER_LAUNCH, **kw))
    stream = torch.cuda.ExternalStream(e.stream, device=dev)
    e.step(STEPS, counters=False)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    groups = torch.randint(0, G, (N,), dtype=torch.int64, device=dev, generator=gen)
    cmds = torch.randint(1, 2 ** 31 - 1, (N,), dtype=torch.int32, device=dev, generator=gen)
    tickets = torch.zeros(N * 4, dtype=torch.int32, device=dev)
    records = torch.zeros(N * 4, dtype=torch.int32, device=dev)
    ld = e.leaders()
    led = float((ld["leader"] >= 0).mean())
    replicas = torch.from_numpy(np.maximum(ld["leader"], 0).astype(np.int32)).to(dev)[groups].contiguous()
    torch.cuda.synchronize(dev)
    base = {"groups": G, "replicas": R, "log_cap": CAP, "steps": STEPS, "messages": N, "reps": REPS,
            "groups_with_leader": round(led, 4), "library_src": abi.build_ids()["library_source_id"]}

    def emit(name, med, all_ms, **more):
        print(json.dumps({"what": name, **base, "median_ms": round(med, 4), "all_ms": [round(x, 4) for x in all_ms],
                          "messages_per_s": round(N / med * 1e3), **more}), flush=True)

    gp, cp, rp, tp, sp = (t.data_ptr() for t in (groups, cmds, replicas, tickets, records))
    bucketed, all_b = timed(stream, lambda: e.append_command_batch_dev(gp, rp, cp, N), REPS)
    emit("append_command_batch_dev (bucketed, the default)", bucketed, all_b)
    e.set_batch_path(abi.BATCH_PATH_SORTED)
    srt, all_s = timed(stream, lambda: e.append_command_batch_dev(gp, rp, cp, N), REPS)
    emit("append_command_batch_dev (sorted)", srt, all_s)
    e.set_batch_path(abi.BATCH_PATH_AUTO)
    prop, all_p = timed(stream, lambda: e.propose_dev(gp, cp, tp, N), REPS)
    st = np.bincount(tickets.cpu().numpy().view(abi.TICKET_DTYPE)["status"], minlength=4).tolist()
    emit("propose_batch_dev", prop, all_p, over_command_batch=round(prop / bucketed, 2),
         over_sorted_command_batch=round(prop / srt, 2), ticket_statuses=st,
         extra_bytes_per_message=R * 32 + 16)
    e.step(10, counters=False)                                     # some of the last batch commits
    res, all_r = timed(stream, lambda: e.resolve_dev(gp, tp, cp, sp, N), REPS)
    rs = np.bincount(records.cpu().numpy().view(abi.TICKET_STATE_DTYPE)["status"], minlength=6).tolist()
    per_ticket = 28 + 16 + R * 3 * 32
    bound_ms = N * per_ticket / HBM_BYTES_PER_S * 1e3
    emit("resolve_tickets_dev", res, all_r, tickets_per_s=round(N / res * 1e3), bytes_per_ticket=per_ticket,
         byte_bound_ms=round(bound_ms, 4), over_bound=round(res / bound_ms, 2), record_statuses=rs,
         device_bytes=e.device_bytes)
    e.close()


if __name__ == "__main__":
    main()
