"""Time the safety audit (raft_audit_observe, raft_audit_report_dev) at the
bench size: 10^6 x 5 under config 3's fault mix (abi.CONFIGS[3]: drops,
isolation churn, commands), flat log, after AUDIT_STEPS steps (default 40).
  observe (first)   from the zero ledger: every group with a committed prefix
                    records its anchor (the second slot read, both header
                    stores, every pair stored).  The ledger is reset, untimed,
                    before each repetition
  observe (steady)  again with no step in between: every check runs, nothing
                    is stored
both against raft_engine_resolve_tickets_dev with one ticket per group in the
same run (it reads the same two state sectors and one log sector per replica)
and against the byte bound at HBM's 8 TB/s: per group R x (three 32-B sectors,
plus a log sector when C > 0) + 2 x (32 + 8 R) B of ledger.
  report_dev        with no group, every 100th group and every group flagged
                    (flags stored with raft_audit_write), against
                    raft_engine_poll_leaders_dev at matching event counts in
                    the same run (the watch's `seen` pairs set with write_watch).

Discipline: one untimed rehearsal per call (it allocates the staging), then
AUDIT_REPS timed calls (default 5), each between events on the engine stream;
medians.  Prints one JSON line per measurement and writes them to AUDIT_OUT
(default profiles/audit_probe/audit_probe.jsonl)."""
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
G = int(os.environ.get("AUDIT_G", "1000000"))
REPS = int(os.environ.get("AUDIT_REPS", "5"))
STEPS = int(os.environ.get("AUDIT_STEPS", "40"))
CAP = int(os.environ.get("AUDIT_LOG_CAP", "64"))
OUT = os.environ.get("AUDIT_OUT", os.path.join(ROOT, "profiles", "audit_probe", "audit_probe.jsonl"))
HBM_BYTES_PER_S = 8e12


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
    e = RaftEngine(abi.make_params(log_cap=CAP, steps_per_launch=STEPS, **kw))
    stream = torch.cuda.ExternalStream(e.stream, device=dev)
    a = e.audit()
    e.step(STEPS, counters=False)
    e.sync()
    base = {"groups": G, "replicas": R, "log_cap": CAP, "steps": STEPS, "reps": REPS,
            "library_source_id": abi.build_ids()["library_source_id"]}
    lines = []

    def emit(name, med, all_ms, **more):
        lines.append(json.dumps({"what": name, **base, "median_ms": round(med, 4),
                                 "all_ms": [round(x, 4) for x in all_ms], **more}))
        print(lines[-1], flush=True)

    # ---- resolve: one ticket per group (replica 0's entry 0)
    groups = torch.arange(G, dtype=torch.int64, device=dev)
    tk = np.zeros(G, dtype=abi.TICKET_DTYPE)
    tk["term"], tk["status"] = 1, abi.PROPOSE_ACCEPTED
    tickets = torch.from_numpy(tk.view(np.int32).reshape(G, 4)).to(dev)
    cmds = torch.zeros(G, dtype=torch.int32, device=dev)
    recs = torch.zeros((G, 4), dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    res_ms, res_all = timed(stream, lambda: e.resolve_dev(groups.data_ptr(), tickets.data_ptr(), cmds.data_ptr(),
                                                          recs.data_ptr(), G), REPS)
    emit("resolve_tickets_dev (one ticket per group)", res_ms, res_all)

    # ---- observe
    infos = []
    first_ms, first_all = timed(stream, lambda: infos.append(a.observe()), REPS, before=a.reset)
    anchored = int((a.read()[:, 4] > 0).sum())
    ledger_b = 32 + 8 * R

    def bound(with_anchor):
        return (G * (R * 96 + 2 * ledger_b) + with_anchor * R * 32) / HBM_BYTES_PER_S * 1e3

    emit("observe (first: every anchor advances)", first_ms, first_all, anchored_groups=anchored, last_info=infos[-1],
         bound_ms=round(bound(0) + anchored * 32 / HBM_BYTES_PER_S * 1e3, 4), over_resolve=round(first_ms / res_ms, 3))
    infos.clear()
    steady_ms, steady_all = timed(stream, lambda: infos.append(a.observe()), REPS)
    b = bound(anchored)
    emit("observe (steady: nothing to advance)", steady_ms, steady_all, anchored_groups=anchored, last_info=infos[-1],
         bound_ms=round(b, 4), over_bound=round(steady_ms / b, 2), over_resolve=round(steady_ms / res_ms, 3))

    # ---- report_dev against poll_leaders_dev at matching event counts
    out = torch.zeros((G, 4), dtype=torch.int32, device=dev)
    wout = torch.zeros((G, 6), dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    clean = a.read()
    clean[:, 0] = 0
    e.poll_leaders(peek=True)
    unseen = e.read_watch()
    e.poll_leaders_dev(wout.data_ptr(), G)
    current = e.read_watch()
    for name, pick in (("no group", slice(0, 0)), ("every 100th group", slice(0, None, 100)), ("every group", slice(None))):
        L = clean.copy()
        L[pick, 0] = abi.AUDIT_TERM_REGRESSED
        a.write(L)
        got = []
        med, all_ms = timed(stream, lambda: got.append(a.report_dev(out.data_ptr(), G)["delivered"]), REPS)
        seen = current.copy()
        seen[pick] = unseen[pick]
        polled = []

        def rewind():
            e.write_watch(seen)

        pmed, pall = timed(stream, lambda: polled.append(e.poll_leaders_dev(wout.data_ptr(), G)["delivered"]), REPS,
                           before=rewind)
        emit(f"report_dev ({name} flagged)", med, all_ms, events=got[-1], bytes_per_event=16)
        emit(f"poll_leaders_dev ({name} changed)", pmed, pall, events=polled[-1], bytes_per_event=24,
             report_over_poll=round(med / pmed, 3))
    a.close()
    e.close()
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
