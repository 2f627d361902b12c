"""Time the linearizable reads (raft_read_begin_batch_dev,
raft_read_serve_batch_dev) at the bench size: config 3 at 10^6 x 5 on a flat
log, a machine of READ_SLOTS (default 8) registers, after READ_STEPS steps
(default 40), one propose of READ_N (default 10^6) uniformly random messages
and one sm_apply; READ_N reads of the same groups from device buffers.

Yardstick: the same library's raft_engine_resolve_tickets_dev on the propose's
tickets at the same n -- the existing call with the same access pattern (a
gather of R state sectors and one log slot per message, one 16-byte record
out).  Each call also gets its byte bound at HBM's 8 TB/s, 32-byte sectors:
  begin    the group twice (the range pass and the begin pass, 8 B each), the R
           quad-0 sectors, quads 1 and 2 of the leader, one log sector, the
           16-byte ticket
  serve    the group, the ticket and the key (28 B), the R quad-0 sectors, one
           head and one register sector, the 16-byte record
  resolve  as scripts/propose_probe.py: 28 B in, 16 B out, per replica two
           state sectors and one log sector

Those are the bytes of a batch in which every ticket is ISSUED.  A message that
finds no leader reads neither quads 1 and 2 nor a log slot, and a ticket that is
not ISSUED (or is malformed) is served from its 28 B of input alone, so each
line also carries the bound weighted by the status mix the run produced
(mix_bytes_per_message, mix_bound_ms, over_mix_bound; the begin's counts a log
sector for the ISSUED tickets only, a TERM_UNCOMMITTED one may have read one too).

Discipline: one untimed rehearsal per call (it allocates the staging), then
READ_REPS timed calls, each between events on the engine stream; medians.
Prints one JSON line per measurement and writes them to READ_OUT (default
profiles/read_probe/read_probe.jsonl)."""
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
G = int(os.environ.get("READ_G", "1000000"))
N = int(os.environ.get("READ_N", "1000000"))
REPS = int(os.environ.get("READ_REPS", "5"))
STEPS = int(os.environ.get("READ_STEPS", "40"))
CAP = int(os.environ.get("READ_LOG_CAP", "300"))
SLOTS = int(os.environ.get("READ_SLOTS", "8"))
OUT = os.environ.get("READ_OUT", os.path.join(ROOT, "profiles", "read_probe", "read_probe.jsonl"))
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


def byte_bounds(R: int) -> dict:
    """Bytes per message each call must move (32-byte sectors)."""
    return {"begin": 2 * 8 + R * 32 + 2 * 32 + 32 + 16, "serve": 28 + R * 32 + 32 + 32 + 16,
            "resolve": 28 + 16 + R * 3 * 32}


def main():
    kw = dict(abi.CONFIGS[3], G=G)
    R = kw["R"]
    dev = torch.device("cuda", 0)
    e = RaftEngine(abi.make_params(log_cap=CAP, steps_per_launch=abi.BENCH_STEPS_PER_LAUNCH, **kw))
    e.sm_configure(SLOTS)
    stream = torch.cuda.ExternalStream(e.stream, device=dev)
    e.step(STEPS, counters=False)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    groups = torch.randint(0, G, (N,), dtype=torch.int64, device=dev, generator=gen)
    cmds = torch.randint(1, 2 ** 31 - 1, (N,), dtype=torch.int32, device=dev, generator=gen)
    keys = torch.randint(0, 2 ** 31 - 1, (N,), dtype=torch.int32, device=dev, generator=gen)
    ptickets, states, rtickets, results = (torch.zeros(N * 4, dtype=torch.int32, device=dev) for _ in range(4))
    torch.cuda.synchronize(dev)
    gp, cp, kp, pp, sp, tp, rp = (t.data_ptr() for t in (groups, cmds, keys, ptickets, states, rtickets, results))
    e.propose_dev(gp, cp, pp, N)
    info = e.sm_apply()
    bounds = byte_bounds(R)
    base = {"groups": G, "replicas": R, "log_cap": CAP, "slots": SLOTS, "steps": STEPS, "messages": N, "reps": REPS,
            "entries_applied": info["applied"], "library_src": abi.build_ids()["library_source_id"]}
    lines = []

    def emit(name, key, med, all_ms, mix_bytes=None, **more):
        bound_ms = N * bounds[key] / HBM_BYTES_PER_S * 1e3
        if mix_bytes is not None:
            mix_ms = mix_bytes / HBM_BYTES_PER_S * 1e3
            more = {"mix_bytes_per_message": round(mix_bytes / N, 1), "mix_bound_ms": round(mix_ms, 4),
                    "over_mix_bound": round(med / mix_ms, 2), **more}
        lines.append(json.dumps({"what": name, **base, "median_ms": round(med, 4), "all_ms": [round(x, 4) for x in all_ms],
                                 "messages_per_s": round(N / med * 1e3), "bytes_per_message": bounds[key],
                                 "byte_bound_ms": round(bound_ms, 4), "over_bound": round(med / bound_ms, 2), **more}))
        print(lines[-1], flush=True)

    res, all_r = timed(stream, lambda: e.resolve_dev(gp, pp, cp, sp, N), REPS)
    rs = np.bincount(states.cpu().numpy().view(abi.TICKET_STATE_DTYPE)["status"], minlength=6).tolist()
    emit("resolve_tickets_dev", "resolve", res, all_r, record_statuses=rs)
    beg, all_b = timed(stream, lambda: e.begin_reads_dev(gp, tp, N), REPS)
    ts = np.bincount(rtickets.cpu().numpy().view(abi.READ_TICKET_DTYPE)["status"], minlength=4).tolist()
    led = N - ts[abi.READ_NO_LEADER]
    begin_mix = N * (2 * 8 + R * 32 + 16) + led * 2 * 32 + ts[abi.READ_ISSUED] * 32
    emit("read_begin_batch_dev", "begin", beg, all_b, mix_bytes=begin_mix, over_resolve=round(beg / res, 2), ticket_statuses=ts)
    srv, all_s = timed(stream, lambda: e.serve_reads_dev(gp, tp, kp, rp, N, check=False), REPS)
    ss = np.bincount(results.cpu().numpy().view(abi.READ_RESULT_DTYPE)["status"], minlength=7).tolist()
    gathered = N - ss[abi.READ_NONE] - ss[abi.READ_INVALID]
    serve_mix = N * (28 + 16) + gathered * (R * 32 + 32 + 32)
    emit("read_serve_batch_dev", "serve", srv, all_s, mix_bytes=serve_mix, over_resolve=round(srv / res, 2), result_statuses=ss,
         return_code=e.last_status, device_bytes=e.device_bytes)
    e.close()
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
