"""Time the scripted network faults (raft_isolate_batch_dev,
raft_engine_heal_network_dev, raft_engine_list_isolated_dev) at the bench size:
config 3 at 10^6 x 5 on a flat log after ISO_STEPS steps (default 40), one
message per group in ascending group order from device buffers.

  isolate   fixed targets (g mod R) and leader-routed ones (NEWEST_LEADER), both
            with RAFT_ISOLATE_REPLACE so that every repetition writes
  heal      a device mask that selects every replica, every group isolated
            before each repetition (untimed)
  list      none / every 100th / every group isolated, into a device buffer

Yardsticks from the same run, not from stored numbers:
  raft_transfer_batch_dev at the same n over the same groups, named targets
  (g mod R) and RAFT_TRANSFER_AUTO: the same shape -- one thread per message, the
  group's role quads, one word written;
  raft_engine_poll_leaders_dev at the same event counts (the watch's pairs are
  rewritten before each repetition, untimed) for the listing;
  each call's byte bound at HBM's 8 TB/s.  The groups ascend, so the bound
  counts coalesced bytes: every array element once per pass that reads it, 16 B
  per state quad touched, 4 B per group word read or written.
    isolate   group, target, steps in both passes (32 B), the claim word cleared,
              min'ed, written back and read (16 B), the isolation word read and
              written (8 B), the ticket (16 B); leader-routed: the R quad-0 (16 R B)
    transfer  group in both passes and the target (20 B), the R quad-0, the
              isolation word (4 B), the ticket (16 B), 4 B per SENT; named: quad
              1 of the target and of the leader (32 B); AUTO: the R quad-1
    heal      the mask byte, the word read, and written where healed
    list      the word in the flag pass; when something is delivered the word
              again, and per record quad 0 of the replica and the 16-B record
    poll      the R quad-0 and the 8-B pair in the flag pass; when something is
              delivered both again, and per event the 24-B record and the pair

Discipline: one untimed rehearsal per call and shape (it allocates the staging
and loads the code objects), then ISO_REPS (default 5) whole calls on the host
clock -- every call ends in a stream synchronize; medians.  Prints one JSON line
per measurement and writes them to ISO_OUT (default
profiles/isolate_probe/isolate_probe.jsonl)."""
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
G = int(os.environ.get("ISO_G", "1000000"))
REPS = int(os.environ.get("ISO_REPS", "5"))
STEPS = int(os.environ.get("ISO_STEPS", "40"))
CAP = int(os.environ.get("ISO_LOG_CAP", "64"))
OUT = os.environ.get("ISO_OUT", os.path.join(ROOT, "profiles", "isolate_probe", "isolate_probe.jsonl"))
HBM_BYTES_PER_S = 8e12
CUT_STEPS = 50


def timed(fn, reps, before=None):
    """Median ms of fn() on the host clock (fn ends in a stream synchronize),
    after one rehearsal; before() runs untimed ahead of every call."""
    out = []
    for k in range(reps + 1):
        if before:
            before()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        if k:
            out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), out


def main():
    kw = dict(abi.CONFIGS[3], G=G)
    R = kw["R"]
    dev = torch.device("cuda", 0)
    e = RaftEngine(abi.make_params(log_cap=CAP, steps_per_launch=abi.BENCH_STEPS_PER_LAUNCH, **kw))
    e.step(STEPS, counters=False)
    groups = torch.arange(G, dtype=torch.int64, device=dev)
    fixed = (groups % R).to(torch.int32)
    newest = torch.full((G,), abi.ISOLATE_NEWEST_LEADER, dtype=torch.int32, device=dev)
    auto = torch.full((G,), abi.TRANSFER_AUTO, dtype=torch.int32, device=dev)
    steps = torch.full((G,), CUT_STEPS, dtype=torch.int32, device=dev)
    every100 = torch.arange(0, G, 100, dtype=torch.int64, device=dev)
    mask = torch.full((G,), 0xFF, dtype=torch.uint8, device=dev)
    tickets = torch.zeros(G * 4, dtype=torch.int32, device=dev)
    records = torch.zeros(G * 4, dtype=torch.int32, device=dev)
    events = torch.zeros(G * 6, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    gp, fp, np_, ap, sp, hp, mp, tp, rp, ep = (t.data_ptr() for t in (groups, fixed, newest, auto, steps, every100, mask,
                                                                       tickets, records, events))
    base = {"groups": G, "replicas": R, "log_cap": CAP, "steps": STEPS, "messages": G, "reps": REPS,
            "library_src": abi.build_ids()["library_source_id"]}
    lines, med = [], {}

    def emit(name, m, all_ms, items, bound_bytes, **more):
        bound_ms = bound_bytes / HBM_BYTES_PER_S * 1e3
        med[name] = m
        lines.append(json.dumps({"what": name, **base, "median_ms": round(m, 4), "all_ms": [round(x, 4) for x in all_ms],
                                 "items": items, "bound_bytes_per_item": round(bound_bytes / max(items, 1), 1),
                                 "bound_ms": round(bound_ms, 4), "over_bound": round(m / bound_ms, 2), **more}))
        print(lines[-1], flush=True)

    def statuses(dtype, names):
        return np.bincount(tickets.cpu().numpy().view(dtype)["status"], minlength=len(names)).tolist()

    # the yardsticks first (they also warm the clocks): a transfer never reads the word it writes, so it repeats
    for name, targ, extra in (("transfer_batch_dev named", fp, 32), ("transfer_batch_dev auto", ap, 16 * R)):
        m, a = timed(lambda: e.transfer_dev(gp, targ, tp, G), REPS)
        st = statuses(abi.TRANSFER_TICKET_DTYPE, abi.TRANSFER_TICKET_STATUS_NAMES)
        emit(name, m, a, G, G * (20 + 16 * R + 4 + 16 + extra) + 4 * st[abi.TRANSFER_SENT], ticket_statuses=st)

    for name, targ, extra, yard in (("isolate_batch_dev fixed", fp, 0, "transfer_batch_dev named"),
                                    ("isolate_batch_dev newest_leader", np_, 16 * R, "transfer_batch_dev auto")):
        m, a = timed(lambda: e.isolate_dev(gp, targ, sp, tp, G, replace=True), REPS)
        st = statuses(abi.ISOLATE_TICKET_DTYPE, abi.ISOLATE_STATUS_NAMES)
        emit(name, m, a, G, G * (32 + 16 + 4 + 16 + extra) + 4 * st[abi.ISOLATE_SET], ticket_statuses=st,
             over_transfer=round(m / med[yard], 2), claim_table_bytes=16 * G)

    def isolate_all():
        e.isolate_dev(gp, fp, sp, tp, G, replace=True)

    info = {}
    m, a = timed(lambda: info.update(e.heal_network_dev(mp, G)), REPS, before=isolate_all)
    emit("heal_network_dev", m, a, G, G * (1 + 4) + 4 * info["healed"], info=dict(info))

    # the listing and the watch's poll at the same event counts
    e.poll_leaders_dev(ep, G)                                        # everything reported: `cur` is the state's pairs
    cur = e.read_watch()
    changed = np.where(cur[:, :1] >= 0, np.array([[-1, 0]], np.int32), np.array([[0, 1]], np.int32)).astype(np.int32)
    for label, idx in (("none", np.zeros(0, np.int64)), ("every 100th", np.arange(0, G, 100)), ("every", np.arange(G))):
        e.heal_network()
        if len(idx) == G:
            isolate_all()
        elif len(idx):
            e.isolate_dev(hp, fp, sp, tp, len(idx), replace=True)    # target g mod R of the first G / 100 positions: any replica
        k = len(idx)
        m, a = timed(lambda: info.update(e.isolated_dev(rp, G)), REPS)
        assert info["delivered"] == k, (info, k)
        emit(f"list_isolated_dev {label}", m, a, G, 4 * G + (4 * G + 32 * k if k else 0), events=k)

        def rewind():
            seen = cur.copy()
            seen[idx] = changed[idx]
            e.write_watch(seen)

        wi = {}
        pm, pa = timed(lambda: wi.update(e.poll_leaders_dev(ep, G)), REPS, before=rewind)
        assert wi["delivered"] == k, (wi, k)
        per_group = 16 * R + 8
        emit(f"poll_leaders_dev {label}", pm, pa, G, per_group * G + (per_group * G + 32 * k if k else 0), events=k)
        lines.append(json.dumps({"what": f"list over poll, {label}", "ratio": round(m / pm, 2)}))
        print(lines[-1], flush=True)
    e.close()
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
