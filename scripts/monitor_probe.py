"""Time the liveness monitor (raft_monitor_observe, raft_monitor_report_dev) at
the bench size: 10^6 x 5 under config 3's fault mix (abi.CONFIGS[3]: drops,
isolation churn, commands), flat log, after MONITOR_STEPS steps (default 40).
  observe (first)   from the zero ledger: every group without a leader starts
                    its outage, every backlog its stall clock, every group its
                    churn window (all four quads may be stored).  The ledger is
                    reset, untimed, before each repetition
  observe (steady)  again with no step in between: every rule runs, nothing
                    changes, nothing is stored
both against raft_audit_observe (steady) in the same run, by the same method,
and against the byte bound at HBM's 8 TB/s: per group R x three 32-B sectors
(quads 0, 1 and 2; no log slot) + 64 B of ledger read (+ 64 B written when
every quad changes).  The audit's steady bound in that run: R x (three sectors
+ a log sector when C > 0) + (32 + 8 R) B of ledger.
  report_dev        with no group, every 100th group and every group listed
                    (now words stored with raft_monitor_write), against
                    raft_audit_report_dev at the same counts in the same run
                    (flags stored with raft_audit_write).

Discipline: one untimed rehearsal per call (it allocates the staging), then
MONITOR_REPS timed calls (default 5), each between events on the engine stream;
medians.  Prints one JSON line per measurement and writes them to MONITOR_OUT
(default profiles/monitor_probe/monitor_probe.jsonl)."""
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
G = int(os.environ.get("MONITOR_G", "1000000"))
REPS = int(os.environ.get("MONITOR_REPS", "5"))
STEPS = int(os.environ.get("MONITOR_STEPS", "40"))
CAP = int(os.environ.get("MONITOR_LOG_CAP", "64"))
OUT = os.environ.get("MONITOR_OUT", os.path.join(ROOT, "profiles", "monitor_probe", "monitor_probe.jsonl"))
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
    m = e.monitor(leaderless_steps=2, stalled_steps=8, lag_entries=8, churn_terms=3, churn_steps=20)
    a = e.audit()
    e.step(STEPS, counters=False)
    e.sync()
    base = {"groups": G, "replicas": R, "log_cap": CAP, "steps": STEPS, "reps": REPS, "config": m.config,
            "library_source_id": abi.build_ids()["library_source_id"]}
    lines = []

    def emit(name, med, all_ms, **more):
        lines.append(json.dumps({"what": name, **base, "median_ms": round(med, 4),
                                 "all_ms": [round(x, 4) for x in all_ms], **more}))
        print(lines[-1], flush=True)

    ms = lambda nbytes: nbytes / HBM_BYTES_PER_S * 1e3

    # ---- the audit's steady observe, the yardstick
    a.observe()
    infos = []
    audit_ms, audit_all = timed(stream, lambda: infos.append(a.observe()), REPS)
    anchored = int((a.read()[:, 4] > 0).sum())
    audit_bound = ms(G * (R * 96 + 32 + 8 * R) + anchored * R * 32)
    emit("audit observe (steady)", audit_ms, audit_all, anchored_groups=anchored, last_info=infos[-1],
         bound_ms=round(audit_bound, 4), over_bound=round(audit_ms / audit_bound, 2))

    # ---- observe
    infos.clear()
    first_ms, first_all = timed(stream, lambda: infos.append(m.observe()), REPS, before=m.reset)
    emit("monitor observe (first: from the zero ledger)", first_ms, first_all, last_info=infos[-1],
         bound_ms=round(ms(G * (R * 96 + 128)), 4), over_bound=round(first_ms / ms(G * (R * 96 + 128)), 2),
         over_audit_steady=round(first_ms / audit_ms, 3))
    infos.clear()
    steady_ms, steady_all = timed(stream, lambda: infos.append(m.observe()), REPS)
    bound = ms(G * (R * 96 + 64))
    emit("monitor observe (steady: nothing stored)", steady_ms, steady_all, last_info=infos[-1],
         bound_ms=round(bound, 4), over_bound=round(steady_ms / bound, 2), over_audit_steady=round(steady_ms / audit_ms, 3))

    # ---- report_dev against the audit's at the same counts
    out = torch.zeros((G, 8), dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    mclean, aclean = m.read(), a.read()
    mclean[:, 0], aclean[:, 0] = 0, 0
    for name, pick in (("no group", slice(0, 0)), ("every 100th group", slice(0, None, 100)), ("every group", slice(None))):
        L, A = mclean.copy(), aclean.copy()
        L[pick, 0] = abi.MONITOR_COMMIT_STALLED
        A[pick, 0] = abi.AUDIT_TERM_REGRESSED
        m.write(L)
        a.write(A)
        got, agot = [], []
        med, all_ms = timed(stream, lambda: got.append(m.report_dev(out.data_ptr(), G)["delivered"]), REPS)
        amed, aall = timed(stream, lambda: agot.append(a.report_dev(out.data_ptr(), G)["delivered"]), REPS)
        emit(f"monitor report_dev ({name} listed)", med, all_ms, events=got[-1], bytes_per_event=32)
        emit(f"audit report_dev ({name} flagged)", amed, aall, events=agot[-1], bytes_per_event=16,
             monitor_over_audit=round(med / amed, 3))
    m.close()
    a.close()
    e.close()
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
