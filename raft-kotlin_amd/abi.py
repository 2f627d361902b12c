"""ctypes mirror of include/raft_engine.h (the engine's C-ABI).

Pure data definitions: structs, constants, and the loader of the HIP engine
library.  The loader never falls back to anything: if the in-tree
``lib/libraft_engine.so`` is missing it raises, so a GPU run cannot silently
take another path.
"""
from __future__ import annotations

import ctypes as C
import os
import warnings

import numpy as np

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
# RAFT_ENGINE_LIB selects an alternative in-tree build (tuning experiments only)
LIB_PATH = os.environ.get("RAFT_ENGINE_LIB") or os.path.join(PKG_DIR, "lib", "libraft_engine.so")

RAFT_OK = 0
RAFT_EINVAL = -1
RAFT_ENOMEM = -2
RAFT_EDEVICE = -3
RAFT_ERANGE = -4
RAFT_ENODEV = -5
RAFT_EWINDOW = -6
RAFT_EFULL = -7
COMM_ID_BYTES = 128          # include/raft_engine.h RAFT_COMM_ID_BYTES

# enum class State (RaftServer.kt:24-26)
FOLLOWER, CANDIDATE, LEADER = 0, 1, 2
MAX_R = 8

CMD_LOWEST_LEADER = 0
CMD_ALL_LEADERS = 1
MODE_REFERENCE = 0
MODE_TEXTBOOK = 1

COUNTER_NAMES = [
    "leaders", "groups_with_leader", "timeouts", "rounds", "votes_granted",
    "leaders_elected", "sessions_ticked", "append_sent", "append_skipped",
    "entries_acked", "commits", "msg_dropped", "commands", "commit_regressions",
    "dual_leader_groups", "log_overflow", "prev_reads_leader",
    "entry_reads_leader", "prev_reads_follower", "entry_writes", "vote_log_reads", "log_window_miss",
]
NUM_COUNTERS = len(COUNTER_NAMES)
COUNTER_STRIDE = 32
MAX_STEPS_PER_LAUNCH = 16384          # include/raft_engine.h RAFT_MAX_STEPS_PER_LAUNCH
# the longest launch whose counter rows stay in LDS for the whole launch
# (raft_engine.hip LDS_MAX_STEPS); a longer one runs as 400-step epochs when
# its schedule is balanced on one sub-range in the reference mode (not a
# partitions-only kernel), else the engine cuts it to this
LDS_MAX_STEPS_PER_LAUNCH = 512
# bench.py's launch length for the step kernels built for 7 waves per SIMD
# (R <= 5, or R = 7 without drops; RAFT_STEP_WAVES_PER_EU in raft_engine.hip):
# the longest that keeps 7 step workgroups per CU within the LDS (STEP_K_7WG,
# 429 steps).  The other kernels run 6 workgroups per CU at any length and
# take the longest LDS launch.
BENCH_STEPS_PER_LAUNCH = 400
# bench.py's launch length where the engine runs epochs: the whole default run
# in one launch (a launch boundary costs ~36 us / sqrt(K) of the waves'
# uneven work; an epoch boundary only waits for a workgroup's own waves)
LONG_STEPS_PER_LAUNCH = 10_000


# The network faults (and command harness) a step kernel is built for
# (raft_step.h NET_*): at R = 3, 5, 7 the engine runs a kernel for drops +
# isolation churn without partitions with config 3's command harness (lowest
# LEADER, no limit), or for partitions alone (configs 5, 2, 1), the other
# checks compiled out; else the NET_ALL kernel
NET_DROP, NET_PART, NET_ISO, NET_CMDLOW = 1, 2, 4, 8
NET_ALL = NET_DROP | NET_PART | NET_ISO


def step_net(R: int, drop_ppm: int = 0, partition_period: int = 0, partition_len: int = 0,
             churn_ppm: int = 0, iso_written: bool = False, cmd_mode: int = 0, cmd_limit: int = 0) -> int:
    """The NET of the step kernel the engine launches (raft_engine.hip step_fn);
    iso_written: an isolation word was written into the state."""
    drops, parts = drop_ppm > 0, partition_period > 0 and partition_len > 0
    iso = churn_ppm > 0 or iso_written
    cmdlow = cmd_mode == CMD_LOWEST_LEADER and cmd_limit == 0
    if R in (3, 5, 7):
        if drops and not parts and cmdlow:
            return NET_DROP | NET_ISO | NET_CMDLOW
        if not drops and not iso:
            return NET_PART
    return NET_ALL


def step_net_of(kw: dict) -> int:
    """step_net of a raft_params keyword dict (abi.CONFIGS entries)."""
    return step_net(kw["R"], kw.get("drop_ppm", 0), kw.get("partition_period", 0), kw.get("partition_len", 0),
                    kw.get("churn_ppm", 0), cmd_mode=kw.get("cmd_mode", CMD_LOWEST_LEADER),
                    cmd_limit=kw.get("cmd_limit", 0))


def bench_steps_per_launch(R: int, mode: int = 0, log_window: int = 0, net: int = NET_ALL, groups: int = 0,
                           simds: int = 1024) -> int:
    """Default fused launch length of bench.py for a kernel variant:
    LONG_STEPS_PER_LAUNCH where the engine runs a long launch as epochs (the
    reference mode, one launch sub-range -- not a partitions-only kernel --
    and a balanced schedule: more chunks of 64 // R groups than the resident
    wave slots of `simds` SIMDs); else 400 for the 7-waves-per-SIMD kernels (R
    <= 5, or R = 7 built for partitions only; either protocol mode, flat log or
    ring), the longest LDS launch for the others."""
    seven = R <= 5 or (R == 7 and net == NET_PART)
    balanced = -(-groups // (64 // R)) > simds * (7 if seven else 6)
    if mode == MODE_REFERENCE and net != NET_PART and balanced:
        return LONG_STEPS_PER_LAUNCH
    return BENCH_STEPS_PER_LAUNCH if seven else LDS_MAX_STEPS_PER_LAUNCH
MAX_AE_ENTRIES = 8           # include/raft_engine.h RAFT_MAX_AE_ENTRIES
C_INDEX = {n: i for i, n in enumerate(COUNTER_NAMES)}

FIELD_NAMES = ["term", "voted", "role", "commit", "last", "phys",
               "election_ms", "flags", "phase_ms", "retry_ms"]
NUM_FIELDS = len(FIELD_NAMES)
# the engine's HBM state per replica: 4 quads of int32 (the 10 fields, the
# log-tail cache and the primary session column; raft_step.h FIELD_SLOT), and
# per group: 3 harness words
REPLICA_STATE_BYTES, GROUP_STATE_BYTES = 64, 12
F_INDEX = {n: i for i, n in enumerate(FIELD_NAMES)}
FL_ARMED, FL_ELECTING, FL_PENDING_RST, FL_HB_ACTIVE, FL_BACKOFF = 1, 2, 4, 8, 16
GROUP_EXTRA = 2


def group_words(R: int) -> int:
    return R * NUM_FIELDS + 2 * R * R + GROUP_EXTRA


class raft_params(C.Structure):
    _fields_ = [
        ("R", C.c_int32), ("log_cap", C.c_int32), ("G", C.c_int64), ("g0", C.c_int64),
        ("seed", C.c_uint64),
        ("heartbeat_ms", C.c_int32), ("election_min_ms", C.c_int32), ("election_max_ms", C.c_int32),
        ("backoff_min_ms", C.c_int32), ("backoff_max_ms", C.c_int32),
        ("round_timeout_ms", C.c_int32), ("retry_ms", C.c_int32),
        ("drop_ppm", C.c_uint32), ("churn_ppm", C.c_uint32), ("churn_steps", C.c_int32),
        ("partition_period", C.c_int32), ("partition_len", C.c_int32),
        ("cmd_ppm", C.c_uint32), ("cmd_mode", C.c_int32), ("cmd_limit", C.c_int32),
        ("steps_per_launch", C.c_int32), ("mode", C.c_int32), ("log_window", C.c_int32),
        ("ae_max_entries", C.c_int32), ("subranges", C.c_int32), ("schedule", C.c_int32),
        ("schedule_workgroups", C.c_int32), ("kernel", C.c_int32),
    ]


# step-kernel schedules (raft_params.schedule)
SCHED_AUTO, SCHED_ONE_PER_WAVE, SCHED_BALANCED = 0, 1, 2
# step-kernel variant (raft_params.kernel): built for the workload, or the general one
KERNEL_AUTO, KERNEL_GENERAL = 0, 1
# raft_engine_set_batch_path
BATCH_PATH_AUTO, BATCH_PATH_SORTED, BATCH_PATH_BUCKETED = 0, 1, 2


class raft_kernel_info(C.Structure):
    _fields_ = [("net", C.c_int32), ("textbook", C.c_int32), ("ring", C.c_int32), ("steps", C.c_int32),
                ("workgroups", C.c_int32), ("resident_workgroups", C.c_int32), ("balanced", C.c_int32),
                ("subranges", C.c_int32), ("reserved", C.c_int32 * 4)]


class raft_vote_req(C.Structure):
    _fields_ = [("term", C.c_int32), ("candidate_id", C.c_int32),
                ("last_log_index", C.c_int32), ("last_log_term", C.c_int32)]


class raft_vote_resp(C.Structure):
    _fields_ = [("term", C.c_int32), ("vote_granted", C.c_int32)]


class raft_append_req(C.Structure):
    _fields_ = [("term", C.c_int32), ("leader_id", C.c_int32), ("prev_log_index", C.c_int32),
                ("prev_log_term", C.c_int32), ("has_entry", C.c_int32), ("entry_term", C.c_int32),
                ("entry_cmd", C.c_uint32), ("leader_commit", C.c_int32)]


class raft_append_resp(C.Structure):
    _fields_ = [("term", C.c_int32), ("success", C.c_int32), ("status", C.c_int32)]


class raft_applied_entry(C.Structure):
    _fields_ = [("group", C.c_int64), ("replica", C.c_int32), ("index", C.c_int32), ("term", C.c_int32),
                ("cmd", C.c_uint32)]


class raft_drain_info(C.Structure):
    _fields_ = [("delivered", C.c_int64), ("pending", C.c_int64), ("lost", C.c_int64), ("regressed", C.c_int64)]


# raft_applied_entry as a numpy record (24 bytes, no padding)
APPLIED_DTYPE = np.dtype([("group", np.int64), ("replica", np.int32), ("index", np.int32), ("term", np.int32),
                          ("cmd", np.uint32)])


class raft_leader_info(C.Structure):
    _fields_ = [("leader", C.c_int32), ("term", C.c_int32), ("n_leaders", C.c_int32), ("commit", C.c_int32)]


class raft_ticket(C.Structure):
    _fields_ = [("replica", C.c_int32), ("index", C.c_int32), ("term", C.c_int32), ("status", C.c_int32)]


class raft_ticket_state(C.Structure):
    _fields_ = [("status", C.c_int32), ("holders", C.c_int32), ("committed_on", C.c_int32), ("unknown", C.c_int32)]


# the client path's records as numpy records (16 bytes each, no padding)
LEADER_DTYPE = np.dtype([("leader", np.int32), ("term", np.int32), ("n_leaders", np.int32), ("commit", np.int32)])
TICKET_DTYPE = np.dtype([("replica", np.int32), ("index", np.int32), ("term", np.int32), ("status", np.int32)])
TICKET_STATE_DTYPE = np.dtype([("status", np.int32), ("holders", np.int32), ("committed_on", np.int32),
                               ("unknown", np.int32)])
# raft_ticket.status (RAFT_PROPOSE_*) and raft_ticket_state.status (RAFT_TICKET_*)
PROPOSE_ACCEPTED, PROPOSE_GHOSTED, PROPOSE_NO_LEADER, PROPOSE_LOG_FULL = 0, 1, 2, 3
TICKET_NONE, TICKET_COMMITTED, TICKET_PENDING, TICKET_LOST, TICKET_UNKNOWN, TICKET_INVALID = 0, 1, 2, 3, 4, 5
TICKET_STATUS_NAMES = ["NONE", "COMMITTED", "PENDING", "LOST", "UNKNOWN", "INVALID"]


class raft_sm_info(C.Structure):
    _fields_ = [("applied", C.c_int64), ("lost", C.c_int64), ("regressed", C.c_int64), ("reserved", C.c_int64)]


class raft_sm_head(C.Structure):
    _fields_ = [("applied", C.c_int32), ("lost", C.c_int32), ("hash", C.c_uint64)]


class raft_sm_value(C.Structure):
    _fields_ = [("value", C.c_uint32), ("replica", C.c_int32), ("applied", C.c_int32), ("commit", C.c_int32)]


# the state machine's records as numpy records (16 bytes each, no padding)
SM_HEAD_DTYPE = np.dtype([("applied", np.int32), ("lost", np.int32), ("hash", np.uint64)])
SM_VALUE_DTYPE = np.dtype([("value", np.uint32), ("replica", np.int32), ("applied", np.int32), ("commit", np.int32)])
SM_SLOTS = (1, 2, 4, 8, 16, 32, 64)      # raft_engine_sm_configure: registers per replica


class raft_restart_info(C.Structure):
    _fields_ = [("restarted", C.c_int64), ("leaders", C.c_int64), ("entries_dropped", C.c_int64),
                ("reserved", C.c_int64)]


# raft_engine_restart*: flags, the largest down_steps, the Philox purposes (RAFT_RNG_*)
RESTART_AMNESIA, RESTART_REPLAY = 1, 2
RESTART_MAX_DOWN_STEPS = (1 << 23) - 1
RNG_TIMER, RNG_RESTART = 1, 7


class raft_install_info(C.Structure):
    _fields_ = [("installed", C.c_int64), ("slots_copied", C.c_int64), ("no_leader", C.c_int64),
                ("leader_gapped", C.c_int64), ("ahead", C.c_int64), ("reserved", C.c_int64 * 3)]


# raft_engine_install_snapshot*: the info as a numpy record (64 bytes, no padding)
INSTALL_INFO_DTYPE = np.dtype([("installed", np.int64), ("slots_copied", np.int64), ("no_leader", np.int64),
                               ("leader_gapped", np.int64), ("ahead", np.int64), ("reserved", np.int64, (3,))])
INSTALL_INFO_FIELDS = ("installed", "slots_copied", "no_leader", "leader_gapped", "ahead")


class raft_read_ticket(C.Structure):
    _fields_ = [("replica", C.c_int32), ("term", C.c_int32), ("read_index", C.c_int32), ("status", C.c_int32)]


class raft_read_result(C.Structure):
    _fields_ = [("value", C.c_uint32), ("status", C.c_int32), ("applied", C.c_int32), ("agree", C.c_int32)]


# linearizable reads: the records as numpy records (16 bytes each, no padding), raft_read_ticket.status and
# raft_read_result.status (RAFT_READ_*)
READ_TICKET_DTYPE = np.dtype([("replica", np.int32), ("term", np.int32), ("read_index", np.int32), ("status", np.int32)])
READ_RESULT_DTYPE = np.dtype([("value", np.uint32), ("status", np.int32), ("applied", np.int32), ("agree", np.int32)])
READ_ISSUED, READ_TERM_UNCOMMITTED, READ_NO_LEADER, READ_UNKNOWN = 0, 1, 2, 3
READ_TICKET_STATUS_NAMES = ["ISSUED", "TERM_UNCOMMITTED", "NO_LEADER", "UNKNOWN"]
READ_SERVED, READ_BEHIND, READ_GAPPED, READ_NO_QUORUM, READ_DEPOSED, READ_NONE, READ_INVALID = 0, 1, 2, 3, 4, 5, 6
READ_STATUS_NAMES = ["SERVED", "BEHIND", "GAPPED", "NO_QUORUM", "DEPOSED", "NONE", "INVALID"]


class raft_transfer_ticket(C.Structure):
    _fields_ = [("from", C.c_int32), ("term", C.c_int32), ("target", C.c_int32), ("status", C.c_int32)]


class raft_transfer_state(C.Structure):
    _fields_ = [("status", C.c_int32), ("leader", C.c_int32), ("term", C.c_int32), ("reserved", C.c_int32)]


class raft_evacuate_info(C.Structure):
    _fields_ = [("led", C.c_int64), ("sent", C.c_int64), ("no_target", C.c_int64), ("behind", C.c_int64),
                ("busy", C.c_int64), ("reserved", C.c_int64 * 3)]


# leadership transfer: the records as numpy records (16 bytes each, no padding), raft_transfer_ticket.status and
# raft_transfer_state.status (RAFT_TRANSFER_*)
TRANSFER_TICKET_DTYPE = np.dtype([("from", np.int32), ("term", np.int32), ("target", np.int32), ("status", np.int32)])
TRANSFER_STATE_DTYPE = np.dtype([("status", np.int32), ("leader", np.int32), ("term", np.int32), ("reserved", np.int32)])
TRANSFER_AUTO = -1
(TRANSFER_SENT, TRANSFER_NO_LEADER, TRANSFER_SELF, TRANSFER_BEHIND, TRANSFER_BUSY, TRANSFER_UNREACHABLE,
 TRANSFER_NO_TARGET, TRANSFER_INVALID) = range(8)
TRANSFER_TICKET_STATUS_NAMES = ["SENT", "NO_LEADER", "SELF", "BEHIND", "BUSY", "UNREACHABLE", "NO_TARGET", "INVALID"]
TRANSFER_COMPLETED, TRANSFER_PENDING, TRANSFER_SUPERSEDED, TRANSFER_NONE = 0, 1, 2, 3
TRANSFER_STATE_NAMES = {0: "COMPLETED", 1: "PENDING", 2: "SUPERSEDED", 3: "NONE", 7: "INVALID"}
EVACUATE_INFO_FIELDS = ("led", "sent", "no_target", "behind", "busy")


class raft_noop_info(C.Structure):
    _fields_ = [("appended", C.c_int64), ("current", C.c_int64), ("no_leader", C.c_int64), ("log_full", C.c_int64),
                ("ghosted", C.c_int64), ("reserved", C.c_int64 * 3)]


# leader no-op entries (raft_engine_append_noops*): the ticket status of a group whose leader's last entry is of
# its own term already (RAFT_PROPOSE_CURRENT, beside PROPOSE_* above), the info as a numpy record (64 bytes, no
# padding)
PROPOSE_CURRENT = 4
NOOP_CMD = 0                 # RaftEngine.append_noops' default command id (any u32 the caller's commands never use)
PROPOSE_STATUS_NAMES = ["ACCEPTED", "GHOSTED", "NO_LEADER", "LOG_FULL", "CURRENT"]
NOOP_INFO_DTYPE = np.dtype([("appended", np.int64), ("current", np.int64), ("no_leader", np.int64),
                            ("log_full", np.int64), ("ghosted", np.int64), ("reserved", np.int64, (3,))])
NOOP_INFO_FIELDS = ("appended", "current", "no_leader", "log_full", "ghosted")


class raft_leader_event(C.Structure):
    _fields_ = [("group", C.c_int64), ("leader", C.c_int32), ("term", C.c_int32), ("prev_leader", C.c_int32),
                ("prev_term", C.c_int32)]


class raft_watch_info(C.Structure):
    _fields_ = [("delivered", C.c_int64), ("pending", C.c_int64), ("gained", C.c_int64), ("lost", C.c_int64),
                ("moved", C.c_int64), ("reterm", C.c_int64), ("leaderless", C.c_int64), ("reserved", C.c_int64)]


# the leader watch (raft_engine_poll_leaders*): raft_leader_event as a numpy record (24 bytes, no padding), the
# info as one (64 bytes), a `seen` pair before the first report
EVENT_DTYPE = np.dtype([("group", np.int64), ("leader", np.int32), ("term", np.int32), ("prev_leader", np.int32),
                        ("prev_term", np.int32)])
WATCH_INFO_DTYPE = np.dtype([("delivered", np.int64), ("pending", np.int64), ("gained", np.int64), ("lost", np.int64),
                             ("moved", np.int64), ("reterm", np.int64), ("leaderless", np.int64),
                             ("reserved", np.int64)])
WATCH_INFO_FIELDS = ("delivered", "pending", "gained", "lost", "moved", "reterm", "leaderless")
WATCH_UNSEEN = (-1, 0)


class raft_outbox_info(C.Structure):
    _fields_ = [(k, C.c_int64) for k in ("queued", "committed", "expired", "deferred", "pending", "orphaned", "unknown",
                                         "retried", "accepted", "ghosted", "no_leader", "log_full", "left")] + [
        ("age_hist", C.c_int64 * 32)]


# the proposal outbox (raft_engine_outbox_*, raft_outbox_submit*): raft_outbox_entry (48 bytes) and raft_outbox_done
# (32 bytes) as numpy records without padding, the scalar fields of raft_outbox_info, the status words
OUTBOX_ENTRY_DTYPE = np.dtype([("tag", np.int64), ("born", np.int64), ("group", np.int32), ("cmd", np.uint32),
                               ("replica", np.int32), ("index", np.int32), ("term", np.int32), ("status", np.int32),
                               ("tries", np.int32), ("pad", np.int32)])
OUTBOX_DONE_DTYPE = np.dtype([("tag", np.int64), ("group", np.int32), ("status", np.int32), ("index", np.int32),
                              ("term", np.int32), ("tries", np.int32), ("age", np.int32)])
OUTBOX_INFO_FIELDS = ("queued", "committed", "expired", "deferred", "pending", "orphaned", "unknown", "retried",
                      "accepted", "ghosted", "no_leader", "log_full", "left")
OUTBOX_NEW, OUTBOX_COMMITTED, OUTBOX_EXPIRED = -1, 1, 2
OUTBOX_DONE_NAMES = {1: "COMMITTED", 2: "EXPIRED"}


class raft_audit_info(C.Structure):
    _fields_ = [(k, C.c_int64) for k in ("newly_flagged", "flagged", "term_regressed", "vote_changed", "two_leaders",
                                         "commit_changed", "leader_incomplete", "unknown")]


class raft_audit_event(C.Structure):
    _fields_ = [("group", C.c_int64), ("flags", C.c_int32), ("first_step", C.c_int32)]


class raft_audit_report_info(C.Structure):
    _fields_ = [("delivered", C.c_int64), ("pending", C.c_int64), ("flagged", C.c_int64), ("reserved", C.c_int64 * 5)]


# the safety audit (raft_audit_*): the sticky flag bits in the order of raft_audit_info's per-kind counts,
# raft_audit_event as a numpy record (16 bytes, no padding), the words of a group's exported ledger
AUDIT_TERM_REGRESSED, AUDIT_VOTE_CHANGED, AUDIT_TWO_LEADERS, AUDIT_COMMIT_CHANGED, AUDIT_LEADER_INCOMPLETE = \
    1, 2, 4, 8, 16
AUDIT_KINDS = ("term_regressed", "vote_changed", "two_leaders", "commit_changed", "leader_incomplete")
AUDIT_ALL = 31
AUDIT_INFO_FIELDS = ("newly_flagged", "flagged") + AUDIT_KINDS + ("unknown",)
AUDIT_REPORT_FIELDS = ("delivered", "pending", "flagged")
AUDIT_EVENT_DTYPE = np.dtype([("group", np.int64), ("flags", np.int32), ("first_step", np.int32)])
AUDIT_WORDS = ("flags", "first_step", "lead_term", "lead_replica", "anchor_count", "anchor_term", "anchor_cmd",
               "anchor_seen_term")
AUDIT_HEAD = len(AUDIT_WORDS)


def audit_words(R: int) -> int:
    """int32 words of one group's exported ledger (raft_audit_read)."""
    return AUDIT_HEAD + 2 * R


class raft_monitor_config(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("leaderless_steps", "stalled_steps", "lag_entries", "churn_terms",
                                         "churn_steps")] + [("reserved", C.c_int32 * 3)]


class raft_monitor_info(C.Structure):
    _fields_ = [(k, C.c_int64) for k in ("flagged", "newly_flagged", "cleared", "leaderless", "commit_stalled", "lagging",
                                         "churning", "down", "outages_ended", "down_steps_ended")] + [
        ("reserved", C.c_int64 * 2)]


class raft_monitor_event(C.Structure):
    _fields_ = [("group", C.c_int64)] + [(k, C.c_int32) for k in ("now", "ever", "down_since", "stall_since", "leader",
                                                                  "lag_mask")]


class raft_monitor_report_info(C.Structure):
    _fields_ = [("delivered", C.c_int64), ("pending", C.c_int64), ("flagged", C.c_int64), ("reserved", C.c_int64 * 5)]


class raft_monitor_availability(C.Structure):
    _fields_ = [("hist", C.c_int64 * 32), ("outages", C.c_int64), ("down_steps", C.c_int64), ("reserved", C.c_int64 * 2)]


# the liveness monitor (raft_monitor_*): the bits of a ledger's now / ever words in the order of raft_monitor_info's
# per-kind counts, the report's word selector, raft_monitor_event as a numpy record (32 bytes, no padding), the
# thresholds of a config, the names of a group's 16 exported ledger words
MONITOR_LEADERLESS, MONITOR_COMMIT_STALLED, MONITOR_LAGGING, MONITOR_CHURNING = 1, 2, 4, 8
MONITOR_KINDS = ("leaderless", "commit_stalled", "lagging", "churning")
MONITOR_ALL = 15
MONITOR_NOW, MONITOR_EVER = 0, 1
MONITOR_INFO_FIELDS = ("flagged", "newly_flagged", "cleared") + MONITOR_KINDS + ("down", "outages_ended",
                                                                               "down_steps_ended")
MONITOR_REPORT_FIELDS = ("delivered", "pending", "flagged")
MONITOR_EVENT_DTYPE = np.dtype([("group", np.int64), ("now", np.int32), ("ever", np.int32), ("down_since", np.int32),
                                ("stall_since", np.int32), ("leader", np.int32), ("lag_mask", np.int32)])
MONITOR_CONFIG_FIELDS = ("leaderless_steps", "stalled_steps", "lag_entries", "churn_terms", "churn_steps")
MONITOR_STALLED_STEPS = 16   # RaftEngine.monitor's default stalled_steps
MONITOR_WORD_NAMES = ("now", "ever", "first_step", "leader", "down_since", "outages", "down_total", "longest",
                      "stall_since", "stall_mark", "win_start", "win_term", "lag_mask", "max_lag", "reserved0",
                      "reserved1")
MONITOR_WORDS = 16
MONITOR_HIST = 32


class raft_wal_cursor(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("term", "vote", "stable", "stable_term", "floor", "pad")]


class raft_wal_record(C.Structure):
    _fields_ = [("group", C.c_int32), ("replica", C.c_int16), ("kind", C.c_int16), ("index", C.c_int32),
                ("term", C.c_int32), ("cmd", C.c_uint32), ("aux", C.c_int32)]


class raft_wal_info(C.Structure):
    _fields_ = [(k, C.c_int64) for k in ("delivered", "pending", "hardstates", "truncates", "entries", "lost",
                                         "regressed")]


# the persistence stream (raft_wal_*): the record kinds, raft_wal_record and raft_wal_cursor as numpy records (24
# bytes each, no padding), the fields of raft_wal_info, a fresh cursor
WAL_HARDSTATE, WAL_TRUNCATE, WAL_ENTRY = 0, 1, 2
WAL_KIND_NAMES = ["HARDSTATE", "TRUNCATE", "ENTRY"]
WAL_RECORD_DTYPE = np.dtype([("group", np.int32), ("replica", np.int16), ("kind", np.int16), ("index", np.int32),
                             ("term", np.int32), ("cmd", np.uint32), ("aux", np.int32)])
WAL_CURSOR_DTYPE = np.dtype([("term", np.int32), ("vote", np.int32), ("stable", np.int32), ("stable_term", np.int32),
                             ("floor", np.int32), ("pad", np.int32)])
WAL_INFO_FIELDS = ("delivered", "pending", "hardstates", "truncates", "entries", "lost", "regressed")
WAL_FRESH = (0, -1, 0, 0, 0, 0)


class raft_isolate_ticket(C.Structure):
    _fields_ = [("replica", C.c_int32), ("steps", C.c_int32), ("status", C.c_int32), ("prev", C.c_int32)]


class raft_heal_info(C.Structure):
    _fields_ = [("healed", C.c_int64), ("idle", C.c_int64), ("kept", C.c_int64), ("reserved", C.c_int64)]


class raft_isolated(C.Structure):
    _fields_ = [("group", C.c_int64), ("replica", C.c_int16), ("role", C.c_int16), ("remaining", C.c_int32)]


class raft_isolated_info(C.Structure):
    _fields_ = [("delivered", C.c_int64), ("pending", C.c_int64), ("running", C.c_int64), ("reserved", C.c_int64)]


# scripted network faults (raft_isolate_batch*, raft_engine_heal_network*, raft_engine_list_isolated*): the leader
# selectors of a target, the flag, the largest steps, raft_isolate_ticket.status, the ticket and raft_isolated as
# numpy records (16 bytes each, no padding), the fields of the two infos
ISOLATE_NEWEST_LEADER, ISOLATE_LOWEST_LEADER = -1, -2
ISOLATE_REPLACE = 1
ISOLATE_MAX_STEPS = (1 << 23) - 1
ISOLATE_SET, ISOLATE_BUSY, ISOLATE_NO_LEADER, ISOLATE_DUPLICATE, ISOLATE_INVALID = range(5)
ISOLATE_STATUS_NAMES = ["SET", "BUSY", "NO_LEADER", "DUPLICATE", "INVALID"]
ISOLATE_TICKET_DTYPE = np.dtype([("replica", np.int32), ("steps", np.int32), ("status", np.int32), ("prev", np.int32)])
ISOLATED_DTYPE = np.dtype([("group", np.int64), ("replica", np.int16), ("role", np.int16), ("remaining", np.int32)])
HEAL_INFO_FIELDS = ("healed", "idle", "kept")
ISOLATED_INFO_FIELDS = ("delivered", "pending", "running")


# the reference's hard-coded constants
DEFAULTS = dict(
    heartbeat_ms=2000,        # RaftServer.kt:115
    election_min_ms=20000,    # Commons.kt:23
    election_max_ms=23000,
    backoff_min_ms=2000,      # RaftServer.kt:221
    backoff_max_ms=3000,
    round_timeout_ms=25000,   # RaftServer.kt:189, :214
    retry_ms=5000,            # Commons.kt:37
)

# BASELINE.json configs; G/steps are the full sizes
CONFIGS = {
    1: dict(R=5, G=1, seed=1, cmd_ppm=1_000_000, cmd_mode=CMD_LOWEST_LEADER, cmd_limit=1000),
    2: dict(R=3, G=10_000, seed=2, cmd_ppm=250_000, cmd_mode=CMD_LOWEST_LEADER),
    3: dict(R=5, G=1_000_000, seed=3, drop_ppm=50_000, churn_ppm=1_000, churn_steps=15,
            cmd_ppm=250_000, cmd_mode=CMD_LOWEST_LEADER),
    5: dict(R=7, G=100_000, seed=5, partition_period=50, partition_len=25,
            cmd_ppm=1_000_000, cmd_mode=CMD_ALL_LEADERS),
}
CONFIG_STEPS = {1: None, 2: 1_000, 3: 10_000, 5: 10_000}


def make_params(**kw) -> raft_params:
    """raft_params with the reference defaults; keyword overrides."""
    p = raft_params()
    p.R = 5
    p.log_cap = 1024
    p.G = 1
    p.g0 = 0
    p.seed = 1
    for k, v in DEFAULTS.items():
        setattr(p, k, v)
    for k, v in kw.items():
        if not hasattr(p, k):
            raise TypeError(f"unknown raft_params field {k!r}")
        setattr(p, k, v)
    return p


def config_params(cfg: int, **kw) -> raft_params:
    d = dict(CONFIGS[cfg])
    d.update(kw)
    return make_params(**d)


def counters_array(n_steps: int) -> np.ndarray:
    return np.zeros((n_steps, COUNTER_STRIDE), dtype=np.int64)


def ptr(a: np.ndarray, ctype):
    return a.ctypes.data_as(C.POINTER(ctype))


_lib = None


def _missing_entry(name: str):
    def stub(*_a, **_k):
        raise RuntimeError(f"{name} is not in this engine build (RAFT_ENGINE_LIB={os.environ.get('RAFT_ENGINE_LIB')})")
    return stub


def check_build(lib, p: str) -> None:
    """Refuse an engine library that was not built from the sources beside it
    (build.py compiles library_source_id() into it): a stale binary would make
    every measurement and parity result describe other code.  Skipped when
    the sources are absent (an installed library)."""
    from . import build as B
    if not B.sources_present():
        return
    lib.raft_build_source_id.restype = C.c_char_p
    have = lib.raft_build_source_id().decode()
    want = B.library_source_id()
    if have != want:
        raise RuntimeError(f"{p} was built from sources {have}, the working tree is {want}: rebuild it "
                           "(`python raft-kotlin_amd/build.py`)")


def build_ids() -> dict:
    """The loaded library's provenance (include/raft_engine.h raft_build_*)."""
    lib = load_library()
    return {"library_source_id": lib.raft_build_source_id().decode(),
            "kernel_source_id": lib.raft_build_kernel_source_id().decode(),
            "batch_source_id": lib.raft_build_batch_source_id().decode(), "path": LIB_PATH}


def load_library(path: str | None = None):
    """Load the HIP engine.  Raises if it is absent: there is no fallback."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise RuntimeError(
            f"HIP engine library not built: {p} (run `python __graft_entry__.py build` "
            "or `python raft-kotlin_amd/build.py`)")
    lib = C.CDLL(p)
    if path is None and not os.environ.get("RAFT_ENGINE_LIB"):
        check_build(lib, p)
    P, I32, I64, U64 = C.POINTER, C.c_int32, C.c_int64, C.c_uint64
    eng = C.c_void_p
    sig = {
        "raft_params_default": (None, [P(raft_params)]),
        "raft_last_error": (C.c_char_p, []),
        "raft_abi_version": (C.c_int, []),
        "raft_build_source_id": (C.c_char_p, []),
        "raft_build_kernel_source_id": (C.c_char_p, []),
        "raft_build_batch_source_id": (C.c_char_p, []),
        "raft_engine_create": (C.c_int, [P(raft_params), C.c_int, P(eng)]),
        "raft_engine_destroy": (C.c_int, [eng]),
        "raft_engine_step": (C.c_int, [eng, I32, P(I64)]),
        "raft_engine_step_async": (C.c_int, [eng, I32, C.c_void_p]),
        "raft_engine_sync": (C.c_int, [eng]),
        "raft_engine_stream": (C.c_void_p, [eng]),
        "raft_engine_set_kernel_timing": (C.c_int, [eng, C.c_int]),
        "raft_engine_kernel_time": (C.c_int, [eng, P(C.c_double), P(I64)]),
        "raft_engine_timed_span": (C.c_int, [eng, C.c_void_p, P(C.c_double)]),
        "raft_engine_step_index": (I64, [eng]),
        "raft_engine_set_step_index": (C.c_int, [eng, I64]),
        "raft_engine_set_steps_per_launch": (C.c_int, [eng, I32]),
        "raft_engine_set_subranges": (C.c_int, [eng, I32]),
        "raft_engine_subranges": (I32, [eng]),
        "raft_engine_kernel_info": (C.c_int, [eng, P(raft_kernel_info)]),
        "raft_engine_wait_stream": (C.c_int, [eng, C.c_void_p]),
        "raft_engine_set_kernel": (C.c_int, [eng, I32]),
        "raft_engine_set_batch_path": (C.c_int, [eng, I32]),
        "raft_engine_reset": (C.c_int, [eng]),
        "raft_engine_trim_staging": (C.c_int, [eng]),
        "raft_engine_device_bytes": (I64, [eng]),
        "raft_engine_read_state": (C.c_int, [eng, I64, I64, P(I32)]),
        "raft_engine_write_state": (C.c_int, [eng, I64, I64, P(I32)]),
        "raft_engine_read_log": (C.c_int, [eng, I64, I64, P(I32), P(C.c_uint32)]),
        "raft_engine_write_log": (C.c_int, [eng, I64, I64, P(I32), P(C.c_uint32)]),
        "raft_engine_digest": (C.c_int, [eng, P(U64)]),
        "raft_engine_digest_range": (C.c_int, [eng, I64, I64, P(U64)]),
        "raft_engine_check_log_matching": (C.c_int, [eng, I64, I64, P(C.c_uint8), P(I64)]),
        "raft_engine_traffic_probe": (C.c_int, [eng, I32, P(I64), P(I64)]),
        "raft_engine_drain_committed": (C.c_int, [eng, I64, I64, I32, C.c_void_p, I64, P(raft_drain_info)]),
        "raft_engine_drain_committed_dev": (C.c_int, [eng, I64, I64, I32, C.c_void_p, I64, P(raft_drain_info)]),
        "raft_engine_read_applied": (C.c_int, [eng, I64, I64, P(I32)]),
        "raft_engine_write_applied": (C.c_int, [eng, I64, I64, P(I32)]),
        "raft_engine_read_leaders": (C.c_int, [eng, I64, I64, C.c_void_p]),
        "raft_propose_batch": (C.c_int, [eng, C.c_void_p, C.c_void_p, C.c_void_p, I64]),
        "raft_propose_batch_dev": (C.c_int, [eng, C.c_void_p, C.c_void_p, C.c_void_p, I64]),
        "raft_engine_resolve_tickets": (C.c_int, [eng, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, I64]),
        "raft_engine_resolve_tickets_dev": (C.c_int, [eng, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, I64]),
        "raft_engine_sm_configure": (C.c_int, [eng, I32]),
        "raft_engine_sm_apply": (C.c_int, [eng, I64, I64, I32, P(raft_sm_info)]),
        "raft_engine_sm_read": (C.c_int, [eng, I64, I64, C.c_void_p, C.c_void_p]),
        "raft_engine_sm_write": (C.c_int, [eng, I64, I64, C.c_void_p, C.c_void_p]),
        "raft_engine_sm_get": (C.c_int, [eng, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, I64]),
        "raft_engine_sm_check": (C.c_int, [eng, I64, I64, P(C.c_uint8), P(I64)]),
        "raft_engine_restart": (C.c_int, [eng, I64, I64, C.c_void_p, I32, I32, P(raft_restart_info)]),
        "raft_engine_restart_dev": (C.c_int, [eng, I64, I64, C.c_void_p, I32, I32, P(raft_restart_info)]),
        "raft_engine_restart_random": (C.c_int, [eng, I64, I64, C.c_uint32, I32, I32, P(raft_restart_info)]),
        "raft_engine_install_snapshot": (C.c_int, [eng, I64, I64, C.c_void_p, I32, P(raft_install_info)]),
        "raft_engine_install_snapshot_dev": (C.c_int, [eng, I64, I64, C.c_void_p, I32, P(raft_install_info)]),
        "raft_read_begin_batch": (C.c_int, [eng, C.c_void_p, C.c_void_p, I64]),
        "raft_read_begin_batch_dev": (C.c_int, [eng, C.c_void_p, C.c_void_p, I64]),
        "raft_read_serve_batch": (C.c_int, [eng, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, I64]),
        "raft_read_serve_batch_dev": (C.c_int, [eng, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, I64]),
        "raft_transfer_batch": (C.c_int, [eng, C.c_void_p, C.c_void_p, C.c_void_p, I64]),
        "raft_transfer_batch_dev": (C.c_int, [eng, C.c_void_p, C.c_void_p, C.c_void_p, I64]),
        "raft_engine_resolve_transfers": (C.c_int, [eng, C.c_void_p, C.c_void_p, C.c_void_p, I64]),
        "raft_engine_resolve_transfers_dev": (C.c_int, [eng, C.c_void_p, C.c_void_p, C.c_void_p, I64]),
        "raft_engine_evacuate": (C.c_int, [eng, I64, I64, C.c_void_p, P(raft_evacuate_info)]),
        "raft_engine_evacuate_dev": (C.c_int, [eng, I64, I64, C.c_void_p, P(raft_evacuate_info)]),
        "raft_engine_append_noops": (C.c_int, [eng, I64, I64, C.c_uint32, C.c_void_p, C.c_void_p, P(raft_noop_info)]),
        "raft_engine_append_noops_dev": (C.c_int, [eng, I64, I64, C.c_uint32, C.c_void_p, C.c_void_p,
                                                   P(raft_noop_info)]),
        "raft_engine_sm_set_noop": (C.c_int, [eng, C.c_int, C.c_uint32]),
        "raft_engine_poll_leaders": (C.c_int, [eng, I64, I64, C.c_void_p, I64, P(raft_watch_info)]),
        "raft_engine_poll_leaders_dev": (C.c_int, [eng, I64, I64, C.c_void_p, I64, P(raft_watch_info)]),
        "raft_engine_read_watch": (C.c_int, [eng, I64, I64, P(I32)]),
        "raft_engine_write_watch": (C.c_int, [eng, I64, I64, P(I32)]),
        "raft_engine_outbox_configure": (C.c_int, [eng, I64, I32]),
        "raft_outbox_submit": (C.c_int, [eng, C.c_void_p, C.c_void_p, C.c_void_p, I64]),
        "raft_outbox_submit_dev": (C.c_int, [eng, C.c_void_p, C.c_void_p, C.c_void_p, I64]),
        "raft_engine_outbox_pump": (C.c_int, [eng, C.c_void_p, I64, P(I64), P(raft_outbox_info)]),
        "raft_engine_outbox_pump_dev": (C.c_int, [eng, C.c_void_p, I64, P(I64), P(raft_outbox_info)]),
        "raft_engine_outbox_read": (C.c_int, [eng, C.c_void_p, I64, P(I64)]),
        "raft_engine_outbox_write": (C.c_int, [eng, C.c_void_p, I64]),
        "raft_audit_create": (C.c_int, [eng, P(C.c_void_p)]),
        "raft_audit_destroy": (C.c_int, [C.c_void_p]),
        "raft_audit_reset": (C.c_int, [C.c_void_p]),
        "raft_audit_device_bytes": (I64, [C.c_void_p]),
        "raft_audit_observe": (C.c_int, [C.c_void_p, I64, I64, P(raft_audit_info)]),
        "raft_audit_report": (C.c_int, [C.c_void_p, I64, I64, C.c_void_p, I64, P(raft_audit_report_info)]),
        "raft_audit_report_dev": (C.c_int, [C.c_void_p, I64, I64, C.c_void_p, I64, P(raft_audit_report_info)]),
        "raft_audit_read": (C.c_int, [C.c_void_p, I64, I64, P(I32)]),
        "raft_audit_write": (C.c_int, [C.c_void_p, I64, I64, P(I32)]),
        "raft_monitor_create": (C.c_int, [eng, P(raft_monitor_config), P(C.c_void_p)]),
        "raft_monitor_destroy": (C.c_int, [C.c_void_p]),
        "raft_monitor_reset": (C.c_int, [C.c_void_p]),
        "raft_monitor_device_bytes": (I64, [C.c_void_p]),
        "raft_monitor_observe": (C.c_int, [C.c_void_p, I64, I64, P(raft_monitor_info)]),
        "raft_monitor_report": (C.c_int, [C.c_void_p, I64, I64, I32, I32, C.c_void_p, I64, P(raft_monitor_report_info)]),
        "raft_monitor_report_dev": (C.c_int, [C.c_void_p, I64, I64, I32, I32, C.c_void_p, I64,
                                              P(raft_monitor_report_info)]),
        "raft_monitor_get_availability": (C.c_int, [C.c_void_p, P(raft_monitor_availability)]),
        "raft_monitor_set_availability": (C.c_int, [C.c_void_p, P(raft_monitor_availability)]),
        "raft_monitor_read": (C.c_int, [C.c_void_p, I64, I64, P(I32)]),
        "raft_monitor_write": (C.c_int, [C.c_void_p, I64, I64, P(I32)]),
        "raft_wal_create": (C.c_int, [eng, P(C.c_void_p)]),
        "raft_wal_destroy": (C.c_int, [C.c_void_p]),
        "raft_wal_reset": (C.c_int, [C.c_void_p]),
        "raft_wal_device_bytes": (I64, [C.c_void_p]),
        "raft_wal_poll": (C.c_int, [C.c_void_p, I64, I64, I32, C.c_void_p, I64, P(raft_wal_info)]),
        "raft_wal_poll_dev": (C.c_int, [C.c_void_p, I64, I64, I32, C.c_void_p, I64, P(raft_wal_info)]),
        "raft_wal_read": (C.c_int, [C.c_void_p, I64, I64, C.c_void_p]),
        "raft_wal_write": (C.c_int, [C.c_void_p, I64, I64, C.c_void_p]),
        "raft_isolate_batch": (C.c_int, [eng, C.c_void_p, C.c_void_p, C.c_void_p, I32, C.c_void_p, I64]),
        "raft_isolate_batch_dev": (C.c_int, [eng, C.c_void_p, C.c_void_p, C.c_void_p, I32, C.c_void_p, I64]),
        "raft_engine_heal_network": (C.c_int, [eng, I64, I64, C.c_void_p, P(raft_heal_info)]),
        "raft_engine_heal_network_dev": (C.c_int, [eng, I64, I64, C.c_void_p, P(raft_heal_info)]),
        "raft_engine_list_isolated": (C.c_int, [eng, I64, I64, C.c_void_p, I64, P(raft_isolated_info)]),
        "raft_engine_list_isolated_dev": (C.c_int, [eng, I64, I64, C.c_void_p, I64, P(raft_isolated_info)]),
        "raft_comm_get_unique_id": (C.c_int, [P(C.c_uint8)]),
        "raft_comm_create": (C.c_int, [P(C.c_uint8), I32, I32, C.c_int, P(C.c_void_p)]),
        "raft_comm_destroy": (C.c_int, [C.c_void_p]),
        "raft_engine_allreduce_counters": (C.c_int, [eng, C.c_void_p, C.c_void_p, C.c_void_p, I32]),
        "raft_vote_batch": (C.c_int, [eng, P(I64), P(I32), P(raft_vote_req), P(raft_vote_resp), I64]),
        "raft_append_batch": (C.c_int, [eng, P(I64), P(I32), P(raft_append_req), P(raft_append_resp), I64]),
        "raft_append_command_batch": (C.c_int, [eng, P(I64), P(I32), P(C.c_uint32), I64]),
        "raft_vote_batch_dev": (C.c_int, [eng, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, I64]),
        "raft_append_batch_dev": (C.c_int, [eng, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, I64]),
        "raft_append_command_batch_dev": (C.c_int, [eng, C.c_void_p, C.c_void_p, C.c_void_p, I64]),
        "raft_philox4x32_10": (None, [P(C.c_uint32), P(C.c_uint32), P(C.c_uint32)]),
        "raft_host_alloc": (C.c_void_p, [I64]),
        "raft_host_free": (C.c_int, [C.c_void_p]),
        # include/raft_wire.h
        "raft_wire_decode_vote_req": (C.c_int, [P(C.c_uint8), P(I64), I64, P(raft_vote_req)]),
        "raft_wire_encode_vote_req": (I64, [P(raft_vote_req), I64, P(C.c_uint8), I64, P(I64)]),
        "raft_wire_decode_vote_resp": (C.c_int, [P(C.c_uint8), P(I64), I64, P(raft_vote_resp)]),
        "raft_wire_encode_vote_resp": (I64, [P(raft_vote_resp), I64, P(C.c_uint8), I64, P(I64)]),
        "raft_wire_decode_append_req": (C.c_int, [P(C.c_uint8), P(I64), I64, P(raft_append_req), P(I64), P(I32),
                                                  P(I32)]),
        "raft_wire_encode_append_req": (I64, [P(raft_append_req), P(C.c_uint8), P(I64), I64, P(C.c_uint8), I64,
                                              P(I64)]),
        "raft_wire_decode_append_resp": (C.c_int, [P(C.c_uint8), P(I64), I64, P(raft_append_resp)]),
        "raft_wire_encode_append_resp": (I64, [P(raft_append_resp), I64, P(C.c_uint8), I64, P(I64)]),
    }
    for name, (res, args) in sig.items():
        if os.environ.get("RAFT_ENGINE_LIB") and not hasattr(lib, name):
            # an older experimental build (RAFT_ENGINE_LIB) may lack newer
            # entry points: bind a stub that says so when it is called
            warnings.warn(f"{path or os.environ['RAFT_ENGINE_LIB']}: no {name}; calls to it will raise", stacklevel=2)
            setattr(lib, name, _missing_entry(name))
            continue
        f = getattr(lib, name)
        f.restype = res
        f.argtypes = args
    _lib = lib if path is None else _lib
    return lib


# symbols declared in include/*.h (checked by tests/test_abi.py)
EXPORTED_SYMBOLS = [
    "raft_params_default", "raft_last_error", "raft_abi_version", "raft_build_source_id",
    "raft_build_kernel_source_id", "raft_build_batch_source_id", "raft_engine_create",
    "raft_engine_destroy", "raft_engine_step", "raft_engine_step_async", "raft_engine_sync",
    "raft_engine_stream", "raft_engine_set_kernel_timing", "raft_engine_kernel_time", "raft_engine_timed_span",
    "raft_engine_step_index", "raft_engine_set_step_index", "raft_engine_set_steps_per_launch",
    "raft_engine_set_subranges", "raft_engine_subranges", "raft_engine_kernel_info", "raft_engine_wait_stream",
    "raft_engine_set_kernel", "raft_engine_set_batch_path", "raft_engine_reset", "raft_engine_trim_staging",
    "raft_engine_device_bytes",
    "raft_engine_read_state", "raft_engine_write_state", "raft_engine_read_log",
    "raft_engine_write_log", "raft_engine_digest", "raft_engine_digest_range", "raft_engine_check_log_matching", "raft_engine_traffic_probe",
    "raft_engine_drain_committed", "raft_engine_drain_committed_dev", "raft_engine_read_applied", "raft_engine_write_applied",
    "raft_engine_read_leaders", "raft_propose_batch", "raft_propose_batch_dev", "raft_engine_resolve_tickets",
    "raft_engine_resolve_tickets_dev",
    "raft_engine_sm_configure", "raft_engine_sm_apply", "raft_engine_sm_read", "raft_engine_sm_write",
    "raft_engine_sm_get", "raft_engine_sm_check",
    "raft_engine_restart", "raft_engine_restart_dev", "raft_engine_restart_random",
    "raft_engine_install_snapshot", "raft_engine_install_snapshot_dev",
    "raft_read_begin_batch", "raft_read_begin_batch_dev", "raft_read_serve_batch", "raft_read_serve_batch_dev",
    "raft_transfer_batch", "raft_transfer_batch_dev", "raft_engine_resolve_transfers",
    "raft_engine_resolve_transfers_dev", "raft_engine_evacuate", "raft_engine_evacuate_dev",
    "raft_engine_append_noops", "raft_engine_append_noops_dev", "raft_engine_sm_set_noop",
    "raft_engine_poll_leaders", "raft_engine_poll_leaders_dev", "raft_engine_read_watch", "raft_engine_write_watch",
    "raft_engine_outbox_configure", "raft_outbox_submit", "raft_outbox_submit_dev", "raft_engine_outbox_pump",
    "raft_engine_outbox_pump_dev", "raft_engine_outbox_read", "raft_engine_outbox_write",
    "raft_audit_create", "raft_audit_destroy", "raft_audit_reset", "raft_audit_device_bytes", "raft_audit_observe",
    "raft_audit_report", "raft_audit_report_dev", "raft_audit_read", "raft_audit_write",
    "raft_monitor_create", "raft_monitor_destroy", "raft_monitor_reset", "raft_monitor_device_bytes",
    "raft_monitor_observe", "raft_monitor_report", "raft_monitor_report_dev", "raft_monitor_get_availability",
    "raft_monitor_set_availability", "raft_monitor_read", "raft_monitor_write",
    "raft_wal_create", "raft_wal_destroy", "raft_wal_reset", "raft_wal_device_bytes", "raft_wal_poll",
    "raft_wal_poll_dev", "raft_wal_read", "raft_wal_write",
    "raft_isolate_batch", "raft_isolate_batch_dev", "raft_engine_heal_network", "raft_engine_heal_network_dev",
    "raft_engine_list_isolated", "raft_engine_list_isolated_dev",
    "raft_comm_get_unique_id", "raft_comm_create", "raft_comm_destroy", "raft_engine_allreduce_counters", "raft_vote_batch", "raft_append_batch",
    "raft_append_command_batch", "raft_vote_batch_dev", "raft_append_batch_dev", "raft_append_command_batch_dev",
    "raft_philox4x32_10", "raft_host_alloc", "raft_host_free",
    # include/raft_wire.h
    "raft_wire_decode_vote_req", "raft_wire_encode_vote_req", "raft_wire_decode_vote_resp",
    "raft_wire_encode_vote_resp", "raft_wire_decode_append_req", "raft_wire_encode_append_req",
    "raft_wire_decode_append_resp", "raft_wire_encode_append_resp",
]
