"""ctypes mirror of include/raft_engine.h (the engine's C-ABI).

Pure data definitions: structs, constants, and the loader of the HIP engine
library.  The loader never falls back to anything: if the in-tree
``lib/libraft_engine.so`` is missing it raises, so a GPU run cannot silently
take another path.

Every record is declared once, with `record`; its numpy dtype and the tuple
of its scalar fields come from that declaration.  Every entry point is
declared once, in `SIGNATURES`.
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


I16, I32, I64, U32, U64 = C.c_int16, C.c_int32, C.c_int64, C.c_uint32, C.c_uint64


def record(name: str, *groups):
    """The one declaration of a C-ABI record, written like its typedef in the
    header: `groups` are (names, ctype) pairs, names a string of field names
    that share the type, `reserved[3]` for an array.  Returns the
    ctypes.Structure; it carries `dtype`, the same fields as a packed numpy
    dtype (the records that travel as arrays have no padding, so the two agree
    on size and offsets: tests/test_abi.py holds every public *_DTYPE to
    that), and `scalars`, the names of its fields without the
    reserved ones and the arrays (what an info struct becomes a dict of)."""
    fields = []
    for names, ctype in groups:
        for k in names.split():
            k, _, count = k.partition("[")
            fields.append((k, ctype * int(count[:-1]) if count else ctype))
    return type(name, (C.Structure,), {
        "_fields_": fields,
        "dtype": np.dtype([(k, np.dtype(t)) for k, t in fields]),
        "scalars": tuple(k for k, t in fields if not issubclass(t, C.Array) and not k.startswith("reserved"))})


def info_dict(info: C.Structure, fields=None) -> dict:
    """An info struct as a dict of ints: `fields` of it, or its scalar fields."""
    return {k: int(getattr(info, k)) for k in (type(info).scalars if fields is None else fields)}


raft_params = record(
    "raft_params", ("R log_cap", I32), ("G g0", I64), ("seed", U64),
    ("heartbeat_ms election_min_ms election_max_ms backoff_min_ms backoff_max_ms round_timeout_ms retry_ms", I32),
    ("drop_ppm churn_ppm", U32), ("churn_steps partition_period partition_len", I32), ("cmd_ppm", U32),
    ("cmd_mode cmd_limit steps_per_launch mode log_window ae_max_entries subranges schedule schedule_workgroups "
     "kernel", I32))

# step-kernel schedules (raft_params.schedule)
SCHED_AUTO, SCHED_ONE_PER_WAVE, SCHED_BALANCED = 0, 1, 2
# step-kernel variant (raft_params.kernel): built for the workload, or the general one
KERNEL_AUTO, KERNEL_GENERAL = 0, 1
# raft_engine_set_batch_path
BATCH_PATH_AUTO, BATCH_PATH_SORTED, BATCH_PATH_BUCKETED = 0, 1, 2

raft_kernel_info = record("raft_kernel_info", ("net textbook ring steps workgroups resident_workgroups balanced "
                                               "subranges reserved[4]", I32))

# the service boundary's messages (raft_vote_batch*, raft_append_batch*)
raft_vote_req = record("raft_vote_req", ("term candidate_id last_log_index last_log_term", I32))
raft_vote_resp = record("raft_vote_resp", ("term vote_granted", I32))
raft_append_req = record("raft_append_req", ("term leader_id prev_log_index prev_log_term has_entry entry_term", I32),
                         ("entry_cmd", U32), ("leader_commit", I32))
raft_append_resp = record("raft_append_resp", ("term success status", I32))

# committed-entry delivery (raft_engine_drain_committed*): raft_applied_entry is 24 bytes
raft_applied_entry = record("raft_applied_entry", ("group", I64), ("replica index term", I32), ("cmd", U32))
raft_drain_info = record("raft_drain_info", ("delivered pending lost regressed", I64))
APPLIED_DTYPE = raft_applied_entry.dtype

# the client path's records (16 bytes each), raft_ticket.status (RAFT_PROPOSE_*) and raft_ticket_state.status
# (RAFT_TICKET_*)
raft_leader_info = record("raft_leader_info", ("leader term n_leaders commit", I32))
raft_ticket = record("raft_ticket", ("replica index term status", I32))
raft_ticket_state = record("raft_ticket_state", ("status holders committed_on unknown", I32))
LEADER_DTYPE = raft_leader_info.dtype
TICKET_DTYPE = raft_ticket.dtype
TICKET_STATE_DTYPE = raft_ticket_state.dtype
PROPOSE_ACCEPTED, PROPOSE_GHOSTED, PROPOSE_NO_LEADER, PROPOSE_LOG_FULL = 0, 1, 2, 3
TICKET_NONE, TICKET_COMMITTED, TICKET_PENDING, TICKET_LOST, TICKET_UNKNOWN, TICKET_INVALID = 0, 1, 2, 3, 4, 5
TICKET_STATUS_NAMES = ["NONE", "COMMITTED", "PENDING", "LOST", "UNKNOWN", "INVALID"]

# the state machine's records (16 bytes each)
raft_sm_info = record("raft_sm_info", ("applied lost regressed reserved", I64))
raft_sm_head = record("raft_sm_head", ("applied lost", I32), ("hash", U64))
raft_sm_value = record("raft_sm_value", ("value", U32), ("replica applied commit", I32))
SM_HEAD_DTYPE = raft_sm_head.dtype
SM_VALUE_DTYPE = raft_sm_value.dtype
SM_SLOTS = (1, 2, 4, 8, 16, 32, 64)      # raft_engine_sm_configure: registers per replica

# raft_engine_restart*: the info, the flags, the largest down_steps, the Philox purposes (RAFT_RNG_*)
raft_restart_info = record("raft_restart_info", ("restarted leaders entries_dropped reserved", I64))
RESTART_AMNESIA, RESTART_REPLAY = 1, 2
RESTART_MAX_DOWN_STEPS = (1 << 23) - 1
RNG_TIMER, RNG_RESTART = 1, 7

# raft_engine_install_snapshot*: the info (64 bytes)
raft_install_info = record("raft_install_info", ("installed slots_copied no_leader leader_gapped ahead reserved[3]", I64))
INSTALL_INFO_DTYPE = raft_install_info.dtype
INSTALL_INFO_FIELDS = raft_install_info.scalars

# linearizable reads: the records (16 bytes each), raft_read_ticket.status and raft_read_result.status
# (RAFT_READ_*)
raft_read_ticket = record("raft_read_ticket", ("replica term read_index status", I32))
raft_read_result = record("raft_read_result", ("value", U32), ("status applied agree", I32))
READ_TICKET_DTYPE = raft_read_ticket.dtype
READ_RESULT_DTYPE = raft_read_result.dtype
READ_ISSUED, READ_TERM_UNCOMMITTED, READ_NO_LEADER, READ_UNKNOWN = 0, 1, 2, 3
READ_TICKET_STATUS_NAMES = ["ISSUED", "TERM_UNCOMMITTED", "NO_LEADER", "UNKNOWN"]
READ_SERVED, READ_BEHIND, READ_GAPPED, READ_NO_QUORUM, READ_DEPOSED, READ_NONE, READ_INVALID = 0, 1, 2, 3, 4, 5, 6
READ_STATUS_NAMES = ["SERVED", "BEHIND", "GAPPED", "NO_QUORUM", "DEPOSED", "NONE", "INVALID"]

# leadership transfer: the records (16 bytes each), raft_transfer_ticket.status and raft_transfer_state.status
# (RAFT_TRANSFER_*)
raft_transfer_ticket = record("raft_transfer_ticket", ("from term target status", I32))
raft_transfer_state = record("raft_transfer_state", ("status leader term reserved", I32))
raft_evacuate_info = record("raft_evacuate_info", ("led sent no_target behind busy reserved[3]", I64))
TRANSFER_TICKET_DTYPE = raft_transfer_ticket.dtype
TRANSFER_STATE_DTYPE = raft_transfer_state.dtype
TRANSFER_AUTO = -1
(TRANSFER_SENT, TRANSFER_NO_LEADER, TRANSFER_SELF, TRANSFER_BEHIND, TRANSFER_BUSY, TRANSFER_UNREACHABLE,
 TRANSFER_NO_TARGET, TRANSFER_INVALID) = range(8)
TRANSFER_TICKET_STATUS_NAMES = ["SENT", "NO_LEADER", "SELF", "BEHIND", "BUSY", "UNREACHABLE", "NO_TARGET", "INVALID"]
TRANSFER_COMPLETED, TRANSFER_PENDING, TRANSFER_SUPERSEDED, TRANSFER_NONE = 0, 1, 2, 3
TRANSFER_STATE_NAMES = {0: "COMPLETED", 1: "PENDING", 2: "SUPERSEDED", 3: "NONE", 7: "INVALID"}
EVACUATE_INFO_FIELDS = raft_evacuate_info.scalars

# leader no-op entries (raft_engine_append_noops*): the info (64 bytes), the ticket status of a group whose
# leader's last entry is of its own term already (RAFT_PROPOSE_CURRENT, beside PROPOSE_* above)
raft_noop_info = record("raft_noop_info", ("appended current no_leader log_full ghosted reserved[3]", I64))
PROPOSE_CURRENT = 4
NOOP_CMD = 0                 # RaftEngine.append_noops' default command id (any u32 the caller's commands never use)
PROPOSE_STATUS_NAMES = ["ACCEPTED", "GHOSTED", "NO_LEADER", "LOG_FULL", "CURRENT"]
NOOP_INFO_DTYPE = raft_noop_info.dtype
NOOP_INFO_FIELDS = raft_noop_info.scalars

# the leader watch (raft_engine_poll_leaders*): raft_leader_event (24 bytes), the info (64 bytes), a `seen` pair
# before the first report
raft_leader_event = record("raft_leader_event", ("group", I64), ("leader term prev_leader prev_term", I32))
raft_watch_info = record("raft_watch_info", ("delivered pending gained lost moved reterm leaderless reserved", I64))
EVENT_DTYPE = raft_leader_event.dtype
WATCH_INFO_DTYPE = raft_watch_info.dtype
WATCH_INFO_FIELDS = raft_watch_info.scalars
WATCH_UNSEEN = (-1, 0)

# the proposal outbox (raft_engine_outbox_*, raft_outbox_submit*): the info, raft_outbox_entry (48 bytes) and
# raft_outbox_done (32 bytes) as numpy records without padding, the status words
raft_outbox_info = record("raft_outbox_info", ("queued committed expired deferred pending orphaned unknown retried "
                                               "accepted ghosted no_leader log_full left age_hist[32]", I64))
OUTBOX_ENTRY_DTYPE = np.dtype([("tag", np.int64), ("born", np.int64), ("group", np.int32), ("cmd", np.uint32),
                               ("replica", np.int32), ("index", np.int32), ("term", np.int32), ("status", np.int32),
                               ("tries", np.int32), ("pad", np.int32)])
OUTBOX_DONE_DTYPE = np.dtype([("tag", np.int64), ("group", np.int32), ("status", np.int32), ("index", np.int32),
                              ("term", np.int32), ("tries", np.int32), ("age", np.int32)])
OUTBOX_INFO_FIELDS = raft_outbox_info.scalars
OUTBOX_NEW, OUTBOX_COMMITTED, OUTBOX_EXPIRED = -1, 1, 2
OUTBOX_DONE_NAMES = {1: "COMMITTED", 2: "EXPIRED"}

# the safety audit (raft_audit_*): the sticky flag bits in the order of raft_audit_info's per-kind counts,
# raft_audit_event (16 bytes), the words of a group's exported ledger
raft_audit_info = record("raft_audit_info", ("newly_flagged flagged term_regressed vote_changed two_leaders "
                                             "commit_changed leader_incomplete unknown", I64))
raft_audit_event = record("raft_audit_event", ("group", I64), ("flags first_step", I32))
raft_audit_report_info = record("raft_audit_report_info", ("delivered pending flagged reserved[5]", I64))
AUDIT_TERM_REGRESSED, AUDIT_VOTE_CHANGED, AUDIT_TWO_LEADERS, AUDIT_COMMIT_CHANGED, AUDIT_LEADER_INCOMPLETE = \
    1, 2, 4, 8, 16
AUDIT_KINDS = raft_audit_info.scalars[2:7]
AUDIT_ALL = 31
AUDIT_INFO_FIELDS = raft_audit_info.scalars
AUDIT_REPORT_FIELDS = raft_audit_report_info.scalars
AUDIT_EVENT_DTYPE = raft_audit_event.dtype
AUDIT_WORDS = ("flags", "first_step", "lead_term", "lead_replica", "anchor_count", "anchor_term", "anchor_cmd",
               "anchor_seen_term")
AUDIT_HEAD = len(AUDIT_WORDS)


def audit_words(R: int) -> int:
    """int32 words of one group's exported ledger (raft_audit_read)."""
    return AUDIT_HEAD + 2 * R


# the liveness monitor (raft_monitor_*): the thresholds of a config, the bits of a ledger's now / ever words in
# the order of raft_monitor_info's per-kind counts, the report's word selector, raft_monitor_event (32 bytes), the
# names of a group's 16 exported ledger words
raft_monitor_config = record("raft_monitor_config", ("leaderless_steps stalled_steps lag_entries churn_terms "
                                                     "churn_steps reserved[3]", I32))
raft_monitor_info = record("raft_monitor_info", ("flagged newly_flagged cleared leaderless commit_stalled lagging "
                                                 "churning down outages_ended down_steps_ended reserved[2]", I64))
raft_monitor_event = record("raft_monitor_event", ("group", I64), ("now ever down_since stall_since leader lag_mask", I32))
raft_monitor_report_info = record("raft_monitor_report_info", ("delivered pending flagged reserved[5]", I64))
raft_monitor_availability = record("raft_monitor_availability", ("hist[32] outages down_steps reserved[2]", I64))
MONITOR_LEADERLESS, MONITOR_COMMIT_STALLED, MONITOR_LAGGING, MONITOR_CHURNING = 1, 2, 4, 8
MONITOR_KINDS = raft_monitor_info.scalars[3:7]
MONITOR_ALL = 15
MONITOR_NOW, MONITOR_EVER = 0, 1
MONITOR_INFO_FIELDS = raft_monitor_info.scalars
MONITOR_REPORT_FIELDS = raft_monitor_report_info.scalars
MONITOR_EVENT_DTYPE = raft_monitor_event.dtype
MONITOR_CONFIG_FIELDS = raft_monitor_config.scalars
MONITOR_STALLED_STEPS = 16   # RaftEngine.monitor's default stalled_steps
MONITOR_WORD_NAMES = ("now", "ever", "first_step", "leader", "down_since", "outages", "down_total", "longest",
                      "stall_since", "stall_mark", "win_start", "win_term", "lag_mask", "max_lag", "reserved0",
                      "reserved1")
MONITOR_WORDS = 16
MONITOR_HIST = 32

# the persistence stream (raft_wal_*): raft_wal_record and raft_wal_cursor (24 bytes each), the info, the record
# kinds, a fresh cursor
raft_wal_cursor = record("raft_wal_cursor", ("term vote stable stable_term floor pad", I32))
raft_wal_record = record("raft_wal_record", ("group", I32), ("replica kind", I16), ("index term", I32), ("cmd", U32),
                         ("aux", I32))
raft_wal_info = record("raft_wal_info", ("delivered pending hardstates truncates entries lost regressed", I64))
WAL_HARDSTATE, WAL_TRUNCATE, WAL_ENTRY = 0, 1, 2
WAL_KIND_NAMES = ["HARDSTATE", "TRUNCATE", "ENTRY"]
WAL_RECORD_DTYPE = raft_wal_record.dtype
WAL_CURSOR_DTYPE = raft_wal_cursor.dtype
WAL_INFO_FIELDS = raft_wal_info.scalars
WAL_FRESH = (0, -1, 0, 0, 0, 0)

# scripted network faults (raft_isolate_batch*, raft_engine_heal_network*, raft_engine_list_isolated*): the ticket
# and raft_isolated (16 bytes each), the two infos, the leader selectors of a target, the flag, the largest steps,
# raft_isolate_ticket.status
raft_isolate_ticket = record("raft_isolate_ticket", ("replica steps status prev", I32))
raft_heal_info = record("raft_heal_info", ("healed idle kept reserved", I64))
raft_isolated = record("raft_isolated", ("group", I64), ("replica role", I16), ("remaining", I32))
raft_isolated_info = record("raft_isolated_info", ("delivered pending running reserved", I64))
ISOLATE_NEWEST_LEADER, ISOLATE_LOWEST_LEADER = -1, -2
ISOLATE_REPLACE = 1
ISOLATE_MAX_STEPS = (1 << 23) - 1
ISOLATE_SET, ISOLATE_BUSY, ISOLATE_NO_LEADER, ISOLATE_DUPLICATE, ISOLATE_INVALID = range(5)
ISOLATE_STATUS_NAMES = ["SET", "BUSY", "NO_LEADER", "DUPLICATE", "INVALID"]
ISOLATE_TICKET_DTYPE = raft_isolate_ticket.dtype
ISOLATED_DTYPE = raft_isolated.dtype
HEAL_INFO_FIELDS = raft_heal_info.scalars
ISOLATED_INFO_FIELDS = raft_isolated_info.scalars


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


def _signatures() -> dict:
    """name -> (restype, argtypes) of every function include/*.h declares
    (tests/test_abi.py holds the keys to the headers)."""
    P, INT, VP, U8 = C.POINTER, C.c_int, C.c_void_p, C.c_uint8
    eng = VP
    batch3 = (INT, [eng, VP, VP, VP, I64])                   # (engine, three device or host vectors, n)
    batch4 = (INT, [eng, VP, VP, VP, VP, I64])
    ranged = (INT, [VP, I64, I64, P(I32)])                   # (handle, g0, n, int32 words)

    def stream(handle, info, *sel):
        """(handle, g0, n, selectors..., records, room, info): an ordered record stream."""
        return (INT, [handle, I64, I64, *sel, VP, I64, P(info)])

    return {
        "raft_params_default": (None, [P(raft_params)]),
        "raft_last_error": (C.c_char_p, []),
        "raft_abi_version": (INT, []),
        "raft_build_source_id": (C.c_char_p, []),
        "raft_build_kernel_source_id": (C.c_char_p, []),
        "raft_build_batch_source_id": (C.c_char_p, []),
        "raft_engine_create": (INT, [P(raft_params), INT, P(eng)]),
        "raft_engine_destroy": (INT, [eng]),
        "raft_engine_step": (INT, [eng, I32, P(I64)]),
        "raft_engine_step_async": (INT, [eng, I32, VP]),
        "raft_engine_sync": (INT, [eng]),
        "raft_engine_stream": (VP, [eng]),
        "raft_engine_set_kernel_timing": (INT, [eng, INT]),
        "raft_engine_kernel_time": (INT, [eng, P(C.c_double), P(I64)]),
        "raft_engine_timed_span": (INT, [eng, VP, P(C.c_double)]),
        "raft_engine_step_index": (I64, [eng]),
        "raft_engine_set_step_index": (INT, [eng, I64]),
        "raft_engine_set_steps_per_launch": (INT, [eng, I32]),
        "raft_engine_set_subranges": (INT, [eng, I32]),
        "raft_engine_subranges": (I32, [eng]),
        "raft_engine_kernel_info": (INT, [eng, P(raft_kernel_info)]),
        "raft_engine_wait_stream": (INT, [eng, VP]),
        "raft_engine_set_kernel": (INT, [eng, I32]),
        "raft_engine_set_batch_path": (INT, [eng, I32]),
        "raft_engine_reset": (INT, [eng]),
        "raft_engine_trim_staging": (INT, [eng]),
        "raft_engine_device_bytes": (I64, [eng]),
        "raft_engine_read_state": ranged,
        "raft_engine_write_state": ranged,
        "raft_engine_read_log": (INT, [eng, I64, I64, P(I32), P(U32)]),
        "raft_engine_write_log": (INT, [eng, I64, I64, P(I32), P(U32)]),
        "raft_engine_digest": (INT, [eng, P(U64)]),
        "raft_engine_digest_range": (INT, [eng, I64, I64, P(U64)]),
        "raft_engine_check_log_matching": (INT, [eng, I64, I64, P(U8), P(I64)]),
        "raft_engine_traffic_probe": (INT, [eng, I32, P(I64), P(I64)]),
        "raft_engine_drain_committed": stream(eng, raft_drain_info, I32),
        "raft_engine_drain_committed_dev": stream(eng, raft_drain_info, I32),
        "raft_engine_read_applied": ranged,
        "raft_engine_write_applied": ranged,
        "raft_engine_read_leaders": (INT, [eng, I64, I64, VP]),
        "raft_propose_batch": batch3,
        "raft_propose_batch_dev": batch3,
        "raft_engine_resolve_tickets": batch4,
        "raft_engine_resolve_tickets_dev": batch4,
        "raft_engine_sm_configure": (INT, [eng, I32]),
        "raft_engine_sm_apply": (INT, [eng, I64, I64, I32, P(raft_sm_info)]),
        "raft_engine_sm_read": (INT, [eng, I64, I64, VP, VP]),
        "raft_engine_sm_write": (INT, [eng, I64, I64, VP, VP]),
        "raft_engine_sm_get": batch4,
        "raft_engine_sm_check": (INT, [eng, I64, I64, P(U8), P(I64)]),
        "raft_engine_restart": (INT, [eng, I64, I64, VP, I32, I32, P(raft_restart_info)]),
        "raft_engine_restart_dev": (INT, [eng, I64, I64, VP, I32, I32, P(raft_restart_info)]),
        "raft_engine_restart_random": (INT, [eng, I64, I64, U32, I32, I32, P(raft_restart_info)]),
        "raft_engine_install_snapshot": (INT, [eng, I64, I64, VP, I32, P(raft_install_info)]),
        "raft_engine_install_snapshot_dev": (INT, [eng, I64, I64, VP, I32, P(raft_install_info)]),
        "raft_read_begin_batch": (INT, [eng, VP, VP, I64]),
        "raft_read_begin_batch_dev": (INT, [eng, VP, VP, I64]),
        "raft_read_serve_batch": batch4,
        "raft_read_serve_batch_dev": batch4,
        "raft_transfer_batch": batch3,
        "raft_transfer_batch_dev": batch3,
        "raft_engine_resolve_transfers": batch3,
        "raft_engine_resolve_transfers_dev": batch3,
        "raft_engine_evacuate": (INT, [eng, I64, I64, VP, P(raft_evacuate_info)]),
        "raft_engine_evacuate_dev": (INT, [eng, I64, I64, VP, P(raft_evacuate_info)]),
        "raft_engine_append_noops": (INT, [eng, I64, I64, U32, VP, VP, P(raft_noop_info)]),
        "raft_engine_append_noops_dev": (INT, [eng, I64, I64, U32, VP, VP, P(raft_noop_info)]),
        "raft_engine_sm_set_noop": (INT, [eng, INT, U32]),
        "raft_engine_poll_leaders": stream(eng, raft_watch_info),
        "raft_engine_poll_leaders_dev": stream(eng, raft_watch_info),
        "raft_engine_read_watch": ranged,
        "raft_engine_write_watch": ranged,
        "raft_engine_outbox_configure": (INT, [eng, I64, I32]),
        "raft_outbox_submit": batch3,
        "raft_outbox_submit_dev": batch3,
        "raft_engine_outbox_pump": (INT, [eng, VP, I64, P(I64), P(raft_outbox_info)]),
        "raft_engine_outbox_pump_dev": (INT, [eng, VP, I64, P(I64), P(raft_outbox_info)]),
        "raft_engine_outbox_read": (INT, [eng, VP, I64, P(I64)]),
        "raft_engine_outbox_write": (INT, [eng, VP, I64]),
        "raft_audit_create": (INT, [eng, P(VP)]),
        "raft_audit_destroy": (INT, [VP]),
        "raft_audit_reset": (INT, [VP]),
        "raft_audit_device_bytes": (I64, [VP]),
        "raft_audit_observe": (INT, [VP, I64, I64, P(raft_audit_info)]),
        "raft_audit_report": stream(VP, raft_audit_report_info),
        "raft_audit_report_dev": stream(VP, raft_audit_report_info),
        "raft_audit_read": ranged,
        "raft_audit_write": ranged,
        "raft_monitor_create": (INT, [eng, P(raft_monitor_config), P(VP)]),
        "raft_monitor_destroy": (INT, [VP]),
        "raft_monitor_reset": (INT, [VP]),
        "raft_monitor_device_bytes": (I64, [VP]),
        "raft_monitor_observe": (INT, [VP, I64, I64, P(raft_monitor_info)]),
        "raft_monitor_report": stream(VP, raft_monitor_report_info, I32, I32),
        "raft_monitor_report_dev": stream(VP, raft_monitor_report_info, I32, I32),
        "raft_monitor_get_availability": (INT, [VP, P(raft_monitor_availability)]),
        "raft_monitor_set_availability": (INT, [VP, P(raft_monitor_availability)]),
        "raft_monitor_read": ranged,
        "raft_monitor_write": ranged,
        "raft_wal_create": (INT, [eng, P(VP)]),
        "raft_wal_destroy": (INT, [VP]),
        "raft_wal_reset": (INT, [VP]),
        "raft_wal_device_bytes": (I64, [VP]),
        "raft_wal_poll": stream(VP, raft_wal_info, I32),
        "raft_wal_poll_dev": stream(VP, raft_wal_info, I32),
        "raft_wal_read": (INT, [VP, I64, I64, VP]),
        "raft_wal_write": (INT, [VP, I64, I64, VP]),
        "raft_isolate_batch": (INT, [eng, VP, VP, VP, I32, VP, I64]),
        "raft_isolate_batch_dev": (INT, [eng, VP, VP, VP, I32, VP, I64]),
        "raft_engine_heal_network": (INT, [eng, I64, I64, VP, P(raft_heal_info)]),
        "raft_engine_heal_network_dev": (INT, [eng, I64, I64, VP, P(raft_heal_info)]),
        "raft_engine_list_isolated": stream(eng, raft_isolated_info),
        "raft_engine_list_isolated_dev": stream(eng, raft_isolated_info),
        "raft_comm_get_unique_id": (INT, [P(U8)]),
        "raft_comm_create": (INT, [P(U8), I32, I32, INT, P(VP)]),
        "raft_comm_destroy": (INT, [VP]),
        "raft_engine_allreduce_counters": (INT, [eng, VP, VP, VP, I32]),
        "raft_vote_batch": (INT, [eng, P(I64), P(I32), P(raft_vote_req), P(raft_vote_resp), I64]),
        "raft_append_batch": (INT, [eng, P(I64), P(I32), P(raft_append_req), P(raft_append_resp), I64]),
        "raft_append_command_batch": (INT, [eng, P(I64), P(I32), P(U32), I64]),
        "raft_vote_batch_dev": batch4,
        "raft_append_batch_dev": batch4,
        "raft_append_command_batch_dev": batch3,
        "raft_philox4x32_10": (None, [P(U32), P(U32), P(U32)]),
        "raft_host_alloc": (VP, [I64]),
        "raft_host_free": (INT, [VP]),
        # include/raft_wire.h
        "raft_wire_decode_vote_req": (INT, [P(U8), P(I64), I64, P(raft_vote_req)]),
        "raft_wire_encode_vote_req": (I64, [P(raft_vote_req), I64, P(U8), I64, P(I64)]),
        "raft_wire_decode_vote_resp": (INT, [P(U8), P(I64), I64, P(raft_vote_resp)]),
        "raft_wire_encode_vote_resp": (I64, [P(raft_vote_resp), I64, P(U8), I64, P(I64)]),
        "raft_wire_decode_append_req": (INT, [P(U8), P(I64), I64, P(raft_append_req), P(I64), P(I32), P(I32)]),
        "raft_wire_encode_append_req": (I64, [P(raft_append_req), P(U8), P(I64), I64, P(U8), I64, P(I64)]),
        "raft_wire_decode_append_resp": (INT, [P(U8), P(I64), I64, P(raft_append_resp)]),
        "raft_wire_encode_append_resp": (I64, [P(raft_append_resp), I64, P(U8), I64, P(I64)]),
    }


SIGNATURES = _signatures()
# symbols declared in include/*.h (checked by tests/test_abi.py)
EXPORTED_SYMBOLS = list(SIGNATURES)

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
    for name, (res, args) in SIGNATURES.items():
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


def bind_extension(lib, signatures: dict, mark: str):
    """What the extension modules (replay.py, debug.py) share: `lib` (None: the
    engine library) with restype and argtypes of `signatures` bound, once per
    library (`mark` is the attribute that remembers it).  There is no fallback:
    a library without one of the entry points raises."""
    lib = lib or load_library()
    if getattr(lib, mark, False):
        return lib
    for name, (res, args) in signatures.items():
        if not hasattr(lib, name):
            raise RuntimeError(f"{name} is not in this engine build: rebuild it (`python raft-kotlin_amd/build.py`)")
        f = getattr(lib, name)
        f.restype, f.argtypes = res, args
    setattr(lib, mark, True)
    return lib
