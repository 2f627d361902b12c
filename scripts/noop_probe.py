"""Time leader no-op entries (raft_engine_append_noops_dev) at the bench size:
10^6 x 5 in RAFT_MODE_TEXTBOOK on a flat log, no commands and no faults, after
NOOP_STEPS steps (default 40: every group has elected a leader whose log holds
no entry of its term).  Two measurements of the call over every group, with
device tickets:
  first   the call that appends: one entry per group with a leader.  It is not
          repeatable as it stands, so before each repetition the state is put
          back (write_state of the words saved before the first call: lastIndex
          returns to where it was, and the appended slot is beyond it again) and
          the log-tail cache the write made stale is rebuilt by an untimed call
          (an evacuate with an empty mask)
  second  the call again: every leader's tail is of its own term, all CURRENT,
          nothing is written but the tickets

Yardstick: raft_engine_evacuate_dev of replica 0 over every group in the same
run, in the state before the first call -- the same shape (one thread per
group, range form, the same leader lookup).  Each call also gets its byte bound
at HBM's 8 TB/s: per group the R quad-0 words (16 B each,
contiguous) and the 20 bytes of its ticket and ticket_cmd; per group with a
leader quads 1 and 2 of that replica (a 32-byte sector each); per append one
sector for the 8-byte slot and the two sectors of the quads that changed.
evacuate's bound is scripts/transfer_probe.py's.

Discipline: one untimed rehearsal per call (it allocates the staging), then
NOOP_REPS timed calls, each between events on the engine stream; medians.
Prints one JSON line per measurement and writes them to NOOP_OUT (default
profiles/noop_probe/noop_probe.jsonl)."""
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

abi = importlib.import_module("raft-kotlin_amd.abi")
RaftEngine = importlib.import_module("raft-kotlin_amd.engine").RaftEngine
G = int(os.environ.get("NOOP_G", "1000000"))
REPS = int(os.environ.get("NOOP_REPS", "7"))
STEPS = int(os.environ.get("NOOP_STEPS", "40"))
CAP = int(os.environ.get("NOOP_LOG_CAP", "64"))
OUT = os.environ.get("NOOP_OUT", os.path.join(ROOT, "profiles", "noop_probe", "noop_probe.jsonl"))
HBM_BYTES_PER_S = 8e12
CMD = 0xFFFF0001
# timers under which every group has a leader within 13 steps (the reference's 20-23 s timeouts over a 2 s
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
    R = 5
    dev = torch.device("cuda", 0)
    e = RaftEngine(abi.make_params(R=R, G=G, seed=3, log_cap=CAP, mode=abi.MODE_TEXTBOOK, ae_max_entries=4, cmd_ppm=0,
                                   steps_per_launch=STEPS, **TIMERS))
    stream = torch.cuda.ExternalStream(e.stream, device=dev)
    e.step(STEPS, counters=False)
    tickets = torch.zeros(G * 4, dtype=torch.int32, device=dev)
    cmds = torch.zeros(G, dtype=torch.int32, device=dev)
    mask = torch.ones(G, dtype=torch.uint8, device=dev)                   # replica 0 of every group
    none = torch.zeros(G, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    tp, cp, mp, zp = (t.data_ptr() for t in (tickets, cmds, mask, none))
    saved = e.read_state()
    base = {"groups": G, "replicas": R, "log_cap": CAP, "steps": STEPS, "reps": REPS, "mode": "textbook",
            "library_src": abi.build_ids()["library_source_id"]}
    lines = []

    def emit(name, med, all_ms, mix_bytes, **more):
        mix_ms = mix_bytes / HBM_BYTES_PER_S * 1e3
        lines.append(json.dumps({"what": name, **base, "median_ms": round(med, 4), "all_ms": [round(x, 4) for x in all_ms],
                                 "groups_per_s": round(G / med * 1e3), "mix_bytes_per_group": round(mix_bytes / G, 1),
                                 "mix_bound_ms": round(mix_ms, 4), "over_mix_bound": round(med / mix_ms, 2), **more}))
        print(lines[-1], flush=True)

    def restore():
        e.write_state(saved)
        e.evacuate_dev(zp, G)                                             # rebuilds the stale log-tail cache, sets no timer
        e.sync()

    # the yardstick first (and the clock warm-up), in the state the first call finds
    info = {}
    evac, all_e = timed(stream, lambda: info.update(e.evacuate_dev(mp, G)), REPS)
    emit("evacuate_dev", evac, all_e, G * (1 + R * 32) + info["led"] * (R * 32 + 32) + info["sent"] * 32, info=dict(info))

    def noop_bytes(i):
        led = G - i["no_leader"]
        return G * (R * 16 + 20) + led * 2 * 32 + (i["appended"] + i["log_full"]) * 3 * 32

    first, all_f = timed(stream, lambda: info.update(e.append_noops_dev(tp, cp, 0, G, CMD)), REPS, before=restore)
    i1 = {k: info[k] for k in abi.NOOP_INFO_FIELDS}
    emit("append_noops_dev first", first, all_f, noop_bytes(i1), over_evacuate=round(first / evac, 2), info=i1)

    second, all_s = timed(stream, lambda: info.update(e.append_noops_dev(tp, cp, 0, G, CMD)), REPS)
    i2 = {k: info[k] for k in abi.NOOP_INFO_FIELDS}
    emit("append_noops_dev second", second, all_s, noop_bytes(i2), over_evacuate=round(second / evac, 2), info=i2)
    e.close()
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
