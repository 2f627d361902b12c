"""Time leadership transfer (raft_transfer_batch_dev,
raft_engine_resolve_transfers_dev, raft_engine_evacuate_dev) at the bench size:
config 3 at 10^6 x 5 on a flat log after XFER_STEPS steps (default 400);
XFER_N (default 10^6) messages with uniformly random groups and targets in
-1..R-1 from device buffers, an evacuate of replica 0 over the whole range, and
once the route the calls replace: read_state -> edit on the host -> write_state
of every group.

Yardstick: the same library's raft_read_begin_batch_dev over the same groups in
the same run -- it reads the same R quad-0 sectors, two more quads of the leader
and one log slot, and stores one 16-byte record.  Each call also gets its byte
bound at HBM's 8 TB/s, 32-byte sectors, for the status mix the run produced:
  transfer  the group twice (the range pass and the transfer pass) and the
            target (20 B), the R quad-0 sectors, the isolation word's sector,
            the 16-byte ticket; quad 1 of the target (AUTO: of the R replicas),
            quad 1 of the leader for a named target other than the leader in a
            group that has one, and one sector written per SENT ticket
  resolve   the group and the ticket (24 B), the 16-byte record, and the R
            quad-0 sectors for a SENT ticket
  evacuate  per group the mask byte and the R quad-0 sectors; for a group led
            from inside the mask the R quad-1 sectors and the isolation word's,
            and one sector written where a timer was set
  begin     as scripts/read_probe.py

Discipline: one untimed rehearsal per call (it allocates the staging), then
XFER_REPS timed calls, each between events on the engine stream; medians.  A
transfer is repeatable: it never reads the word it writes, so every repetition
judges the same state.  Prints one JSON line per measurement and writes them to
XFER_OUT (default profiles/transfer_probe/transfer_probe.jsonl)."""
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
G = int(os.environ.get("XFER_G", "1000000"))
N = int(os.environ.get("XFER_N", "1000000"))
REPS = int(os.environ.get("XFER_REPS", "7"))
STEPS = int(os.environ.get("XFER_STEPS", "400"))
CAP = int(os.environ.get("XFER_LOG_CAP", "300"))
OUT = os.environ.get("XFER_OUT", os.path.join(ROOT, "profiles", "transfer_probe", "transfer_probe.jsonl"))
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
    targets = torch.randint(-1, R, (N,), dtype=torch.int32, device=dev, generator=gen)
    mask = torch.ones(G, dtype=torch.uint8, device=dev)                   # replica 0 of every group
    tickets, states, rtickets = (torch.zeros(N * 4, dtype=torch.int32, device=dev) for _ in range(3))
    torch.cuda.synchronize(dev)
    gp, ap, tp, sp, rp, mp = (t.data_ptr() for t in (groups, targets, tickets, states, rtickets, mask))
    base = {"groups": G, "replicas": R, "log_cap": CAP, "steps": STEPS, "messages": N, "reps": REPS,
            "library_src": abi.build_ids()["library_source_id"]}
    lines = []

    def emit(name, med, all_ms, items, mix_bytes, **more):
        mix_ms = mix_bytes / HBM_BYTES_PER_S * 1e3
        lines.append(json.dumps({"what": name, **base, "median_ms": round(med, 4), "all_ms": [round(x, 4) for x in all_ms],
                                 "items": items, "items_per_s": round(items / med * 1e3),
                                 "mix_bytes_per_item": round(mix_bytes / items, 1), "mix_bound_ms": round(mix_ms, 4),
                                 "over_mix_bound": round(med / mix_ms, 2), **more}))
        print(lines[-1], flush=True)

    # clock warm-up and the yardstick first: begin over the same groups
    beg, all_b = timed(stream, lambda: e.begin_reads_dev(gp, rp, N), REPS)
    ts = np.bincount(rtickets.cpu().numpy().view(abi.READ_TICKET_DTYPE)["status"], minlength=4).tolist()
    led = N - ts[abi.READ_NO_LEADER]
    emit("read_begin_batch_dev", beg, all_b, N, N * (2 * 8 + R * 32 + 16) + led * 2 * 32 + ts[abi.READ_ISSUED] * 32,
         ticket_statuses=ts)

    xfer, all_x = timed(stream, lambda: e.transfer_dev(gp, ap, tp, N), REPS)
    tk = tickets.cpu().numpy().view(abi.TRANSFER_TICKET_DTYPE)
    tgt = targets.cpu().numpy()
    st = np.bincount(tk["status"], minlength=8).tolist()
    named = tgt >= 0
    named_other = int((named & (tk["from"] >= 0) & (tk["status"] != abi.TRANSFER_SELF)).sum())
    xfer_mix = N * (20 + R * 32 + 32 + 16) + int((~named).sum()) * R * 32 + int(named.sum()) * 32 + named_other * 32 + \
        st[abi.TRANSFER_SENT] * 32
    emit("transfer_batch_dev", xfer, all_x, N, xfer_mix, over_begin=round(xfer / beg, 2), ticket_statuses=st)

    res, all_r = timed(stream, lambda: e.resolve_transfers_dev(gp, tp, sp, N), REPS)
    rs = np.bincount(states.cpu().numpy().view(abi.TRANSFER_STATE_DTYPE)["status"], minlength=8).tolist()
    emit("resolve_transfers_dev", res, all_r, N, N * (24 + 16) + st[abi.TRANSFER_SENT] * R * 32,
         over_begin=round(res / beg, 2), state_statuses=rs)

    info = {}
    evac, all_e = timed(stream, lambda: info.update(e.evacuate_dev(mp, G)), REPS)
    emit("evacuate_dev", evac, all_e, G, G * (1 + R * 32) + info["led"] * (R * 32 + 32) + info["sent"] * 32,
         over_begin=round(evac / beg, 2), info=info)

    # the route the calls replace, once: every group's words to the host, the word edited there, and back
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    w = e.read_state()
    t1 = time.perf_counter()
    w[:, 1 * abi.NUM_FIELDS + abi.F_INDEX["election_ms"]] |= 0          # the edit's place; the words stay as they are
    e.write_state(w)
    e.sync()
    t2 = time.perf_counter()
    route_ms = (t2 - t0) * 1e3
    lines.append(json.dumps({"what": "read_state + write_state", **base, "once_ms": round(route_ms, 1),
                             "read_ms": round((t1 - t0) * 1e3, 1), "write_ms": round((t2 - t1) * 1e3, 1),
                             "bytes_each_way": int(w.nbytes), "over_transfer": round(route_ms / xfer, 1),
                             "over_evacuate": round(route_ms / evac, 1)}))
    print(lines[-1], flush=True)
    e.close()
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
