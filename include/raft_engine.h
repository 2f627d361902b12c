/*
 * raft_engine.h — C-ABI of the MI355X batched Raft engine.
 *
 * Drop-in boundary for the consensus core of arodionov/raft-kotlin
 * (reference: src/main/kotlin/ua/org/kug/raft/RaftServer.kt, Commons.kt,
 * src/main/proto/greeter.proto).  The reference exposes one Raft node per JVM
 * process behind the gRPC service
 *
 *     service Raft { rpc Vote(RequestVoteRPC) returns (ResponseVoteRPC);
 *                    rpc Append(RequestAppendEntriesRPC) returns (ResponseAppendEntriesRPC); }
 *                                                             (greeter.proto:46-49)
 *
 * implemented by RaftServer.vote()  (RaftServer.kt:228-251) and
 *                RaftServer.append() (RaftServer.kt:253-287),
 * and drives itself from timers: the election timer (Commons.kt:10-31,
 * RaftServer.kt:180-185), the candidate loop leaderElection()
 * (RaftServer.kt:187-226) and the leader heartbeat/commit loop
 * appendRequestAndLeaderHeartbeat() (RaftServer.kt:109-178).
 *
 * This engine runs that node state machine for G independent groups of R
 * replicas each, in deterministic lockstep (one step = one heartbeat period),
 * with the whole state resident in GPU HBM.  The schedule that turns the
 * racy reference into a deterministic one is specified in DESIGN.md §3.
 *
 * Conventions
 *   - plain C types only; every function returns RAFT_OK (0) or a negative
 *     RAFT_E* code; raft_last_error() gives the text (thread-local).
 *   - the caller owns every host buffer; the engine owns device memory.
 *   - one engine handle is not reentrant: callers serialise per handle.
 *   - the reference's per-message exceptions (Log.get IndexOutOfBounds,
 *     gRPC failures) are per-message status values, never errors.
 */
#ifndef RAFT_ENGINE_H
#define RAFT_ENGINE_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: raft_params.schedule / schedule_workgroups / kernel, automatic
 * subranges by workload (1 or 3), raft_engine_kernel_info, raft_engine_set_kernel,
 * raft_engine_reset, raft_engine_wait_stream.  Added since without a new
 * version, because nothing that existed changed: committed-entry delivery
 * (raft_engine_drain_committed*, raft_engine_read_applied / write_applied), the
 * client path (raft_engine_read_leaders, raft_propose_batch*, raft_engine_resolve_tickets*),
 * the replicated state machine (raft_engine_sm_*), replica restart
 * (raft_engine_restart*), linearizable reads (raft_read_begin_batch*,
 * raft_read_serve_batch*), snapshot install (raft_engine_install_snapshot*),
 * leadership transfer (raft_transfer_batch*, raft_engine_resolve_transfers*,
 * raft_engine_evacuate*), leader no-op entries (raft_engine_append_noops*,
 * raft_engine_sm_set_noop), the leader watch (raft_engine_poll_leaders*,
 * raft_engine_read_watch / write_watch), the proposal outbox
 * (raft_engine_outbox_*, raft_outbox_submit*), the safety audit
 * (raft_audit_*), the liveness monitor (raft_monitor_*), the persistence
 * stream (raft_wal_*) and scripted network faults (raft_isolate_batch*,
 * raft_engine_heal_network*, raft_engine_list_isolated*) */
#define RAFT_ABI_VERSION 2

/* ---- status codes ---------------------------------------------------- */
#define RAFT_OK            0
#define RAFT_EINVAL       -1   /* bad argument                               */
#define RAFT_ENOMEM       -2   /* device/host allocation failed              */
#define RAFT_EDEVICE      -3   /* HIP runtime error                          */
#define RAFT_ERANGE       -4   /* group range outside the engine             */
#define RAFT_ENODEV       -5   /* no HIP device / kernel image unavailable   */
#define RAFT_EWINDOW      -6   /* a handler batch touched a log slot below the
                                * retained window (results invalid, like overflow) */
#define RAFT_EFULL        -7   /* the outbox has no room for the batch: nothing was enqueued */

/* ---- node roles: enum class State (RaftServer.kt:24-26) --------------- */
#define RAFT_FOLLOWER  0
#define RAFT_CANDIDATE 1
#define RAFT_LEADER    2

#define RAFT_MAX_R 8
#define RAFT_MAX_STEPS_PER_LAUNCH 16384 /* steps fused into one kernel launch (beyond 512: epochs) */
#define RAFT_MAX_AE_ENTRIES 8           /* textbook mode: entries one AppendEntries request carries */
#define RAFT_MAX_SUBRANGES 4            /* launch sub-ranges (streams) of the step kernel's grid */

/* ---- command-injection modes (harness) ---------------- */
#define RAFT_CMD_LOWEST_LEADER 0   /* appendCommand on the lowest-id LEADER  */
#define RAFT_CMD_ALL_LEADERS   1   /* appendCommand on every LEADER          */

/* ---- protocol modes -------------------------------- */
#define RAFT_MODE_REFERENCE 0   /* the reference's handlers, quirks Q1-Q14 included (parity) */
#define RAFT_MODE_TEXTBOOK  1   /* opt-in, not the reference: append() rejects a stale term,
                                 * truncates only on conflict and advances the follower commit
                                 * after the consistency check; a new leader starts at
                                 * nextIndex = lastIndex + 1; an acked entry sets
                                 * matchIndex = its index; the leader commit is the median of
                                 * matchIndex[] with a current-term guard */

/*
 * Engine parameters.  The *_ms defaults are the reference's hard-coded
 * constants; raft_params_default() fills them in.
 */
typedef struct raft_params {
    int32_t  R;                 /* replicas per group, 1..8 (servers.size, RaftServer.kt:307)      */
    int32_t  log_cap;           /* physical log slots per replica (ghost tail included, §3.2)      */
    int64_t  G;                 /* groups held by this engine                                      */
    int64_t  g0;                /* global id of this engine's first group (sharding offset)         */
    uint64_t seed;              /* Philox key = (seed lo32, seed hi32)                              */

    int32_t  heartbeat_ms;      /* 2000   fixedRateTimer(period = 2000)   RaftServer.kt:115         */
    int32_t  election_min_ms;   /* 20000  (20_000..23_000).random()       Commons.kt:23             */
    int32_t  election_max_ms;   /* 23000                                                            */
    int32_t  backoff_min_ms;    /* 2000   delay((2_000..3_000).random())  RaftServer.kt:221         */
    int32_t  backoff_max_ms;    /* 3000                                                             */
    int32_t  round_timeout_ms;  /* 25000  countDownLatch.await(25, SECONDS) RaftServer.kt:189,:214  */
    int32_t  retry_ms;          /* 5000   retry(delay = 5000)             Commons.kt:37             */

    uint32_t drop_ppm;          /* Bernoulli drop per request and per response (self never dropped) */
    uint32_t churn_ppm;         /* per group-step probability to isolate the lowest-id LEADER      */
    int32_t  churn_steps;       /* isolation length in steps                                        */
    int32_t  partition_period;  /* 0 = off; else a 2-way partition drawn every period steps ...    */
    int32_t  partition_len;     /* ... holding for partition_len steps                              */
    uint32_t cmd_ppm;           /* per group-step probability of one client command               */
    int32_t  cmd_mode;          /* RAFT_CMD_*                                                       */
    int32_t  cmd_limit;         /* 0 = unlimited, else commands per group                           */
    int32_t  steps_per_launch;  /* engine only: steps fused in one kernel launch, 0..RAFT_MAX_STEPS_PER_LAUNCH (0 = 1);
                                   results never depend on it; <= 429 lets the 7-wave kernels (R <= 5, and
                                   R = 7 without drops) run 7 workgroups per CU (LDS), up to 512 run 6; a
                                   longer balanced launch on one sub-range in the reference mode (not a
                                   partitions-only kernel) runs as 400-step epochs (7 per CU), any other
                                   is cut into launches of 512 */
    int32_t  mode;              /* RAFT_MODE_* (0 = the reference)                                  */
    int32_t  log_window;        /* 0 = every physical slot is kept (log_cap slots per replica);
                                 * else a power of two W <= log_cap: only the newest W physical
                                 * slots [physLen - W, physLen) of each replica are kept, in a ring
                                 * (DESIGN.md §4.2).  Every Log.get / Log.add of the reference below
                                 * physLen - W is counted in RAFT_C_LOG_WINDOW_MISS; a run with a
                                 * miss is invalid (its results are not the reference's), as with
                                 * RAFT_C_LOG_OVERFLOW.  log_cap stays the physLen limit.          */
    int32_t  ae_max_entries;    /* RAFT_MODE_TEXTBOOK only: the entries one AppendEntries request
                                 * carries, nextIndex .. up to ae_max_entries of them
                                 * (greeter.proto:37 `repeated LogEntry entries`).  0 or 1 = one
                                 * entry, the reference's shape (RaftServer.kt:130-132); at most
                                 * RAFT_MAX_AE_ENTRIES.  Must be 0 or 1 in reference mode.       */
    int32_t  subranges;         /* engine only: the step kernel's chunks (waves of groups) split into
                                 * this many contiguous ranges, each launched on its own stream, so
                                 * that one range's last waves can overlap another's next launch.
                                 * 0 = automatic (ABI 2): 1 with the balanced schedule, 3 for a
                                 * partitions-only workload (configs 5, 2, 1), whose automatic
                                 * schedule is one chunk per wave; 1..RAFT_MAX_SUBRANGES.  Results
                                 * never depend on it.                                             */
    int32_t  schedule;          /* engine only: RAFT_SCHED_* (0 = automatic: balanced when the
                                 * chunks outnumber the resident wave slots, except for a
                                 * partitions-only workload).  Results never depend on it.        */
    int32_t  schedule_workgroups; /* engine only: workgroups of a balanced launch (0 = as many as
                                 * the GPU holds at once at the launch's LDS; tests set fewer)     */
    int32_t  kernel;            /* engine only: RAFT_KERNEL_AUTO (0): the step kernel built for the
                                 * configured network faults and command harness (the other checks
                                 * compiled out); RAFT_KERNEL_GENERAL: the kernel that decides every
                                 * fault at run time.  Results never depend on it.                 */
} raft_params;
#define RAFT_KERNEL_AUTO    0
#define RAFT_KERNEL_GENERAL 1

/* ---- step-kernel schedules (raft_params.schedule) --------
 * A chunk is one wave's 64 / R groups.  ONE_PER_WAVE launches a wave per
 * chunk for all steps of the launch: when the chunks outnumber the GPU's
 * resident wave slots, the last round of waves runs on a part-empty chip.
 * BALANCED launches only the workgroups the GPU holds at once (nb of them);
 * workgroup b takes the interleaved chunks b, b + nb, b + 2 nb, ... (so the
 * chunks running at one time are neighbours) and its waves split those
 * chunks' chunk-steps into equal parts (a chunk may pass from one wave to
 * the next between steps), so every wave ends together.  AUTO takes BALANCED when the chunks
 * outnumber the resident wave slots, else ONE_PER_WAVE. */
#define RAFT_SCHED_AUTO         0
#define RAFT_SCHED_ONE_PER_WAVE 1
#define RAFT_SCHED_BALANCED     2   /* whenever every workgroup gets >= 4 chunks */

/* What the last step launch ran (raft_engine_kernel_info). */
typedef struct raft_kernel_info {
    int32_t net;                 /* network faults the kernel was built for: bit 0 drops, 1 partitions,
                                  * 2 isolation churn, 3 config 3's command harness compiled in
                                  * (raft_step.h NET_*)                                              */
    int32_t textbook;            /* 1: RAFT_MODE_TEXTBOOK kernel                                   */
    int32_t ring;                /* 1: the log_window ring kernel                                  */
    int32_t steps;               /* steps of the launch                                            */
    int32_t workgroups;          /* workgroups of the launch, all sub-ranges                       */
    int32_t resident_workgroups; /* workgroups of this kernel the GPU holds at once at that LDS    */
    int32_t balanced;            /* sub-ranges that ran the balanced schedule                      */
    int32_t subranges;           /* sub-ranges (streams) of the launch                             */
    int32_t reserved[4];
} raft_kernel_info;

/* ---- per-step counters (sum over the engine's groups) ------------------ */
enum raft_counter {
    RAFT_C_LEADERS = 0,         /* replicas with role LEADER at step end                        */
    RAFT_C_GROUPS_WITH_LEADER,  /* groups with >= 1 LEADER at step end                          */
    RAFT_C_TIMEOUTS,            /* election timers fired (Commons.kt:25-27)                     */
    RAFT_C_ROUNDS,              /* election rounds started (RaftServer.kt:191-193)              */
    RAFT_C_VOTES_GRANTED,       /* vote() handler grants (RaftServer.kt:237-242)                */
    RAFT_C_LEADERS_ELECTED,     /* heartbeat sessions started (RaftServer.kt:66,:109)           */
    RAFT_C_SESSIONS_TICKED,     /* H: leader ticks that built requests (RaftServer.kt:115-122)  */
    RAFT_C_APPEND_SENT,         /* AppendEntries requests built (incl. self)                    */
    RAFT_C_APPEND_SKIPPED,      /* Q11: Log.get threw while building (RaftServer.kt:128)        */
    RAFT_C_ENTRIES_ACKED,       /* successful entry-carrying responses (RaftServer.kt:157-162)  */
    RAFT_C_COMMITS,             /* commitIndex += 1 by the leader rule (RaftServer.kt:161-162)  */
    RAFT_C_MSG_DROPPED,         /* requests + responses lost (drop mask, isolation, partition)  */
    RAFT_C_COMMANDS,            /* client commands appended (RaftServer.kt:100-107)             */
    RAFT_C_COMMIT_REGRESSIONS,  /* Q4: follower commitIndex decreased (RaftServer.kt:270-272)   */
    RAFT_C_DUAL_LEADER_GROUPS,  /* groups with 2+ LEADERs in one term at step end (safety flag) */
    RAFT_C_LOG_OVERFLOW,        /* Log.add refused for lack of physical capacity (run invalid)  */
    RAFT_C_PREV_READS_LEADER,   /* P_L: log[prev].term reads at the leader                      */
    RAFT_C_ENTRY_READS_LEADER,  /* E_L: log[i-1] reads at the leader                            */
    RAFT_C_PREV_READS_FOLLOWER, /* P_F: log[prev].term reads in append()                        */
    RAFT_C_ENTRY_WRITES,        /* E_W: Log.add stores from append()                            */
    RAFT_C_VOTE_LOG_READS,      /* V: last-log-term reads in the vote path                      */
    RAFT_C_LOG_WINDOW_MISS,     /* Log.get/Log.add below physLen - log_window (run invalid)      */
    RAFT_NUM_COUNTERS
};
#define RAFT_COUNTER_STRIDE 32  /* int64 slots per step in counter buffers */

/* ---- canonical state export ------------------------------------------- */
/*
 * Per-replica scalar fields (int32).  Exported per group as
 *   [R][RAFT_NUM_FIELDS] scalars, then next[R][R], match[R][R] (leader
 *   session of replica s towards replica d at [s][d]), then RAFT_GROUP_EXTRA
 *   harness words; i.e. raft_group_words(R) int32 per group.
 */
enum raft_field {
    RAFT_F_TERM = 0,     /* currentTerm        RaftServer.kt:35-36   */
    RAFT_F_VOTED,        /* votedFor (-1/id)   RaftServer.kt:38-39   */
    RAFT_F_ROLE,         /* state              RaftServer.kt:41-42   */
    RAFT_F_COMMIT,       /* commitIndex        RaftServer.kt:46      */
    RAFT_F_LAST,         /* log.lastIndex      Commons.kt:49         */
    RAFT_F_PHYS,         /* physical ArrayList size (ghost tail)     */
    RAFT_F_ELECTION_MS,  /* election timer remaining (0 if disarmed) */
    RAFT_F_FLAGS,        /* RAFT_FL_* bits below                      */
    RAFT_F_PHASE_MS,     /* round elapsed ms, or backoff remaining    */
    RAFT_F_RETRY_MS,     /* vote retry countdown                      */
    RAFT_NUM_FIELDS
};
#define RAFT_FL_ARMED        (1u << 0)   /* election timer scheduled           */
#define RAFT_FL_ELECTING     (1u << 1)   /* consumer busy in leaderElection()  */
#define RAFT_FL_PENDING_RST  (1u << 2)   /* FOLLOWER send queued while busy    */
#define RAFT_FL_HB_ACTIVE    (1u << 3)   /* heartbeat session running          */
#define RAFT_FL_BACKOFF      (1u << 4)   /* election loop in backoff delay     */
#define RAFT_FL_PENDING_SHIFT 8          /* 8 bits: vote dsts awaiting retry   */
#define RAFT_FL_VOTES_SHIFT   16         /* 4 bits: votesGranted               */
#define RAFT_FL_LATCH_SHIFT   20         /* 4 bits: responses counted on latch */

#define RAFT_GROUP_EXTRA 2   /* [0] isolation word (rem<<8 | replica), [1] commands issued */

static inline int32_t raft_group_words(int32_t R) {
    return R * RAFT_NUM_FIELDS + 2 * R * R + RAFT_GROUP_EXTRA;
}

/* ---- single-handler messages (greeter.proto:16-44, fixed width) -------- */
typedef struct raft_vote_req {       /* RequestVoteRPC  greeter.proto:16-21 */
    int32_t term, candidate_id, last_log_index, last_log_term;
} raft_vote_req;
typedef struct raft_vote_resp {      /* ResponseVoteRPC greeter.proto:23-26 */
    int32_t term, vote_granted;
} raft_vote_resp;
typedef struct raft_append_req {     /* RequestAppendEntriesRPC greeter.proto:28-39 */
    int32_t  term, leader_id, prev_log_index, prev_log_term;
    int32_t  has_entry;              /* entriesCount > 0 (only entries[0] is used, RaftServer.kt:278) */
    int32_t  entry_term;             /* LogEntry.term                          */
    uint32_t entry_cmd;              /* LogEntry.command, interned to a u32 id */
    int32_t  leader_commit;
} raft_append_req;
typedef struct raft_append_resp {    /* ResponseAppendEntriesRPC greeter.proto:41-44 */
    int32_t term, success;
    int32_t status;                  /* 0 ok; 1 = handler threw (Log index < -1), no response */
} raft_append_resp;

typedef struct raft_engine raft_engine;

/* ---- lifecycle -------------------------------------------------------- */
void        raft_params_default(raft_params* p);
const char* raft_last_error(void);
int         raft_abi_version(void);
/* The build's provenance: a short hash of every source, header and compiler
 * flag the library was built from (raft-kotlin_amd/build.py
 * library_source_id; abi.load_library refuses a library whose id differs
 * from the sources beside it), and of the step kernel's three sources
 * (kernel_source_id, the key of bench.py's rocprofv3 rows).  "unknown" for a
 * build made without build.py.  raft_build_batch_source_id: the handler
 * batches' sources and the compile-time knobs that shape their kernels
 * (build.py batch_source_id, the key of their rocprofv3 rows). */
const char* raft_build_source_id(void);
const char* raft_build_kernel_source_id(void);
const char* raft_build_batch_source_id(void);
int raft_engine_create(const raft_params* p, int device, raft_engine** out);
int raft_engine_destroy(raft_engine* e);

/* ---- the hot path ------------------------------------------------------ */
/* Advance every group by n_steps lockstep steps.
 * counters_host: nullable, [n_steps][RAFT_COUNTER_STRIDE] int64, filled in
 * step order.  Synchronous: returns after the device finished. */
int raft_engine_step(raft_engine* e, int32_t n_steps, int64_t* counters_host);
/* Same, asynchronous on the engine stream; counters_dev is a nullable
 * DEVICE pointer to [n_steps][RAFT_COUNTER_STRIDE] int64 (overwritten). */
int raft_engine_step_async(raft_engine* e, int32_t n_steps, int64_t* counters_dev);
int raft_engine_sync(raft_engine* e);
/* hipStream_t of the engine, as void* (for event timing by the caller).  Work
 * enqueued on it after a step_async sees that call's steps finished (state,
 * logs and counter rows).  With launch sub-ranges the step kernels run on the
 * engine's own side streams, which wait for this stream only where an engine
 * call other than a step enqueued work on it: caller work on this stream is
 * ordered before the counter reductions of later steps, not before their
 * step kernels (which touch only engine memory). */
void*   raft_engine_stream(raft_engine* e);
/* Kernel timing: while enabled, every step-kernel launch (of every
 * sub-range) carries its own start / stop timestamps.  raft_engine_kernel_time()
 * synchronises and returns, since the last call, the time during which at
 * least one step kernel ran (the union of the launches' intervals: sub-range
 * launches overlap) and the number of K-step launches of the whole grid, then
 * resets both.  With one sub-range the union is the sum of the launches. */
int raft_engine_set_kernel_timing(raft_engine* e, int enable);
int raft_engine_kernel_time(raft_engine* e, double* total_ms, int64_t* launches);
/* The time from the start of the first step launch timed since timing was
 * switched on (the launch's own start timestamp, carried by the dispatch: no
 * marker ahead of it) to `end_event` (a hipEvent_t the caller recorded after
 * its last launch); call before raft_engine_kernel_time, which resets the
 * timed launches. */
int raft_engine_timed_span(raft_engine* e, void* end_event, double* ms);
int64_t raft_engine_step_index(raft_engine* e);   /* the index of the next step: the steps executed so far
                                                   * (from the index last set), mod 2^32 */
/* Steps fused into one kernel launch from now on (0 = 1), at most
 * RAFT_MAX_STEPS_PER_LAUNCH.  Results do not depend on it. */
int     raft_engine_set_steps_per_launch(raft_engine* e, int32_t k);
/* Launch sub-ranges from now on (raft_params.subranges; 0 = automatic). */
int     raft_engine_set_subranges(raft_engine* e, int32_t n);
int32_t raft_engine_subranges(raft_engine* e);    /* the sub-ranges in use (-1: null engine) */
/* The step kernel and schedule of the last step launch (zeros before the first). */
int     raft_engine_kernel_info(raft_engine* e, raft_kernel_info* out);
/* The step kernel variant from now on (raft_params.kernel).  Results do not
 * depend on it. */
int     raft_engine_set_kernel(raft_engine* e, int32_t kernel);
/* Every group back to the reference's initial state at step 0, exactly as
 * raft_engine_create leaves it (RaftServer.kt:35-48, the election timers armed
 * as init does, :58). */
int     raft_engine_reset(raft_engine* e);
/* Set the index of the next step (its Philox counter c0), 0 <= t < 2^32; with
 * write_state, then write_log, this resumes a run exported at any step.  The
 * index is a 32-bit counter: a run that steps past 2^32 - 1 goes on at 0 (the
 * harness draws, `t % partition_period` and a partition window's first step
 * are all taken in uint32_t), and raft_engine_step_index reports it mod 2^32. */
int     raft_engine_set_step_index(raft_engine* e, int64_t t);
/* HBM owned by the engine: the state, logs, counter buffers, lastApplied and a
 * configured state machine, plus the grow-only staging of the handler batches, accessors, drains and client path (kept for the
 * engine's lifetime at 1.25x the largest request; raft_engine_trim_staging
 * frees it, page-locked host staging included). */
/* ---- multi-GPU: the counter all-reduce ----------------
 * A sharded run is one engine per GPU, each owning a contiguous range of
 * global group ids (raft_params.g0); groups never exchange anything, and the
 * only cross-GPU data is the per-step counter rows, summed over the ranks by
 * RCCL (over xGMI between MI355X GPUs).  Rank 0 makes an id, the caller
 * passes it to every rank (any channel), and each rank creates its
 * communicator (a collective call: it returns once every rank has joined).
 * raft_engine_allreduce_counters enqueues the sum of n_steps counter rows
 * [n_steps][RAFT_COUNTER_STRIDE] int64 (device pointers; in place when
 * out_dev == counters_dev) on the engine's stream, after every step launch
 * already enqueued there.  RCCL is loaded at the first raft_comm call (never
 * for one-GPU use); without it these return RAFT_ENODEV. */
#define RAFT_COMM_ID_BYTES 128
typedef struct raft_comm raft_comm;
int raft_comm_get_unique_id(uint8_t id[RAFT_COMM_ID_BYTES]);
int raft_comm_create(const uint8_t id[RAFT_COMM_ID_BYTES], int32_t nranks, int32_t rank, int device, raft_comm** out);
int raft_comm_destroy(raft_comm* c);
int raft_engine_allreduce_counters(raft_engine* e, raft_comm* c, const int64_t* counters_dev, int64_t* out_dev,
                                   int32_t n_steps);

/* Traffic probe (rocprofv3 calibration; never part of a step): kind 0 moves
 * every chunk's state into registers and back exactly as a step launch's
 * piece entry and exit does (values unchanged); kind 1 makes one 8-byte store
 * per replica into its own log row past its last entry (a flat log only), the
 * Log.add pattern (Commons.kt:56-68).  Kinds 2 and 3 calibrate the handler
 * batches' scattered accesses: 2^21 threads each load (2) or store (3) one
 * 4-byte word in its own 32-byte sector of a 512 MB engine-owned scratch
 * (sectors spread by an odd multiplicative permutation; the state is not
 * touched), counted as 32 bytes per sector.  Returns the bytes the probe's one
 * dispatch reads and writes, so FETCH_SIZE / WRITE_SIZE of that dispatch
 * give the counters' byte factors for the probed access pattern. */
int raft_engine_traffic_probe(raft_engine* e, int32_t kind, int64_t* bytes_read, int64_t* bytes_written);
int64_t raft_engine_device_bytes(raft_engine* e);
int     raft_engine_trim_staging(raft_engine* e);

/* ---- state access (fixtures, parity) ----------------------------------- */
/* out: [n][raft_group_words(R)] int32, canonical layout above. */
int raft_engine_read_state(raft_engine* e, int64_t g0, int64_t n, int32_t* out);
int raft_engine_write_state(raft_engine* e, int64_t g0, int64_t n, const int32_t* in);
/* terms/cmds: [n][R][log_cap], physical slot j at [j].  read_log returns the
 * retained slots [max(0, physLen - W), physLen) and 0 elsewhere.  write_log to
 * a flat log (log_window 0) stores every slot below log_cap; with a
 * log_window W it stores only the slots [max(0, physLen - W), physLen) of the
 * physLen the engine holds at the call, so call write_state first. */
int raft_engine_read_log(raft_engine* e, int64_t g0, int64_t n, int32_t* terms, uint32_t* cmds);
int raft_engine_write_log(raft_engine* e, int64_t g0, int64_t n, const int32_t* terms, const uint32_t* cmds);
/* Order-independent 64-bit digest of the full canonical state and the
 * retained log slots [max(0, physLen - W), physLen) of every replica (W =
 * log_window, or every slot): sum over groups of a per-group hash (DESIGN.md
 * §3 S-13).  digest_range hashes groups [g0, g0 + n) only. */
int raft_engine_digest(raft_engine* e, uint64_t* out);
int raft_engine_digest_range(raft_engine* e, int64_t g0, int64_t n, uint64_t* out);

/* Log Matching over committed prefixes (safety flag): a
 * group of [g0, g0+n) is flagged when two of its replicas hold different
 * (term, cmd) at an index inside both replicas' committed prefixes, i.e.
 * i < min(commitIndex, lastIndex) of each (and, with a log_window, inside
 * both replicas' retained windows).  The reference's quirks (Q4 commit
 * clamp, Q9 no current-term guard) do not preserve this property, so the
 * count is an observation about the reference's protocol, not an engine
 * error.  *mismatched = flagged groups; flags (nullable, host, n bytes)
 * receives 1 per flagged group. */
int raft_engine_check_log_matching(raft_engine* e, int64_t g0, int64_t n, uint8_t* flags, int64_t* mismatched);

/* ---- committed-entry delivery: lastApplied and the apply stream ----------
 * Additive to ABI 2 (RAFT_ABI_VERSION stays 2: nothing that existed changed;
 * a host built against the earlier header runs unchanged).
 *
 * The reference declares lastApplied (RaftServer.kt:47) and never uses it.
 * Here it is a count per replica, like commitIndex: entries [0, lastApplied)
 * of that replica's log have been delivered to the caller.  It lives in an
 * array of its own: it is not part of the canonical state, of read_state /
 * write_state or of the digest, the step kernel never touches it, and
 * raft_engine_create / raft_engine_reset zero it.
 *
 * A drain visits the selected replicas of groups [g0, g0 + n): every replica
 * (replica = -1) or replica index `replica` of each group.  For each, with
 *   hi = clamp(min(commitIndex, lastIndex), 0, log_cap)   (the committed prefix of
 *                                                          raft_engine_check_log_matching)
 *   lo = lastApplied
 * - with a log_window W and wl = max(0, physLen - W): if wl > lo and hi > lo,
 *   the min(wl, hi) - lo entries below the window are gone; they are counted
 *   in `lost`, lo moves past them, and the call returns RAFT_EWINDOW after
 *   doing everything else (as the handler batches do);
 * - if hi < lo (the reference's Q4 clamp can lower commitIndex, an overwrite
 *   can shorten the log) the replica is counted in `regressed`, delivers
 *   nothing and keeps its lastApplied: lastApplied never decreases;
 * - else entries lo .. hi - 1 are delivered, one record each.
 * Records come in ascending (group, replica, index) order.  When there are
 * more than max_entries, exactly the first max_entries of that order are
 * written, lastApplied advances only past what was written (the cut may fall
 * inside one replica's run) and `pending` counts the rest: successive drains
 * concatenated equal one drain with enough room.  out == NULL with
 * max_entries == 0 is a peek: nothing is stored, not even the ring skip, and
 * pending / lost / regressed report what a drain would see.
 *
 * Not promised: in RAFT_MODE_REFERENCE a delivered entry may later be
 * overwritten in the log (quirks Q1-Q4, Q9), and two replicas of one group
 * may deliver different streams.  In RAFT_MODE_TEXTBOOK the streams of a
 * group's replicas are prefixes of one another.
 *
 * Ordering: the call runs on the engine stream; it sees every step enqueued
 * before it and later step launches wait for it.  The host variant returns
 * after the copy; the _dev variant (out: a DEVICE pointer to max_entries
 * records, 8-byte aligned; info stays a host pointer) returns after its
 * kernels finished. */
typedef struct raft_applied_entry {   /* 24 bytes */
    int64_t  group;                   /* engine-local group index */
    int32_t  replica;
    int32_t  index;                   /* log index i; committed when i < min(commitIndex, lastIndex) */
    int32_t  term;
    uint32_t cmd;
} raft_applied_entry;
typedef struct raft_drain_info {      /* 32 bytes */
    int64_t delivered;   /* records written to out */
    int64_t pending;     /* committed, undelivered entries left for lack of room (or all of them, in a peek) */
    int64_t lost;        /* log_window only: entries that left the window undelivered; skipped */
    int64_t regressed;   /* selected replicas whose min(commit, last) < lastApplied */
} raft_drain_info;
/* RAFT_EINVAL: null engine or info, replica outside -1..R-1, max_entries < 0,
 * out == NULL with max_entries > 0; RAFT_ERANGE: groups outside the engine. */
int raft_engine_drain_committed(raft_engine* e, int64_t g0, int64_t n, int32_t replica,
                                raft_applied_entry* out_host, int64_t max_entries, raft_drain_info* info);
int raft_engine_drain_committed_dev(raft_engine* e, int64_t g0, int64_t n, int32_t replica,
                                    raft_applied_entry* out_dev, int64_t max_entries, raft_drain_info* info);
/* lastApplied of groups [g0, g0 + n): [n][R] int32.  write_applied resumes a
 * consumer (with write_state / write_log); every value must be in
 * 0..log_cap, else RAFT_EINVAL and nothing is stored. */
int raft_engine_read_applied(raft_engine* e, int64_t g0, int64_t n, int32_t* out);
int raft_engine_write_applied(raft_engine* e, int64_t g0, int64_t n, const int32_t* in);

/* ---- the client path: leader directory, routed proposals, tickets --------
 * Additive to ABI 2 (RAFT_ABI_VERSION stays 2: nothing that existed changed).
 *
 * The reference's client talks to one node's /cmd/{command} route
 * (RaftServer.kt:87-88), which calls appendCommand (:100-107) on that node,
 * leader or not, and learns nothing about the entry.  Here a client names a
 * group: raft_propose_batch finds the group's leader on the device, runs
 * appendCommand there and returns a ticket (where the entry went);
 * raft_engine_resolve_tickets says later whether that entry is committed,
 * still pending or lost; raft_engine_drain_committed hands the committed
 * entries out.  The canonical state, the digest and the handler batches are
 * untouched by all of this.
 *
 * raft_engine_read_leaders: one 16-byte record per group of [g0, g0 + n), read
 * from the replicas' role words (no whole-state copy).  RAFT_ERANGE: groups
 * outside the engine; RAFT_EINVAL: null engine, or null out_host with n > 0. */
typedef struct raft_leader_info {   /* 16 bytes */
    int32_t leader;     /* lowest replica index whose role is LEADER (RAFT_CMD_LOWEST_LEADER's choice), -1 if none */
    int32_t term;       /* that replica's currentTerm, 0 if none */
    int32_t n_leaders;  /* replicas with role LEADER */
    int32_t commit;     /* that replica's commitIndex, 0 if none */
} raft_leader_info;
int raft_engine_read_leaders(raft_engine* e, int64_t g0, int64_t n, raft_leader_info* out_host);

/* Propose: message m asks for cmd[m] to be replicated in group[m].
 * - Messages apply in batch order.
 * - A group's leader (raft_leader_info.leader) is looked up in the state the
 *   call finds; appendCommand never changes a role, so every message to one
 *   group goes to the same replica, and the k-th accepted message to a group
 *   gets that leader's lastIndex + k.
 * - The effect on state, logs and the log-tail cache is exactly that of
 *   raft_append_command_batch called with those replicas on the messages that
 *   found a leader (the same appendCommand, raft_step.h); a message without a
 *   leader changes nothing.
 * - A group outside the engine fails the whole batch with RAFT_ERANGE before
 *   anything is applied (no ticket is written).  n == 0 is RAFT_OK.  n < 2^31.
 * - With a log_window, a RAFT_MODE_TEXTBOOK add below its replica's window
 *   returns RAFT_EWINDOW after applying the batch, as the handler batches do.
 * - Ordering: the call runs on the engine stream (after rebuilding a stale
 *   log-tail cache), later step launches wait for it, and it returns when the
 *   batch has finished.  The _dev form takes DEVICE pointers under the buffer
 *   rules of raft_*_batch_dev; ticket must be 16-byte aligned.
 * RAFT_EINVAL: null engine, n < 0 or n >= 2^31, a null buffer with n > 0. */
#define RAFT_PROPOSE_ACCEPTED  0  /* stored; log[index] of `replica` is (term, cmd) */
#define RAFT_PROPOSE_GHOSTED   1  /* reference mode only, quirk Q1: physLen != lastIndex before the add, so
                                     log.add stored the entry at the physical end and log[index] shows the
                                     stale slot; lastIndex still grew by one */
#define RAFT_PROPOSE_NO_LEADER 2  /* no replica of the group is LEADER: nothing appended */
#define RAFT_PROPOSE_LOG_FULL  3  /* the leader's Log.add was refused for lack of physical capacity */
typedef struct raft_ticket {      /* 16 bytes */
    int32_t replica;   /* the leader chosen, -1 for NO_LEADER */
    int32_t index;     /* the leader's lastIndex before the add (where the entry went / would have gone), -1 for NO_LEADER */
    int32_t term;      /* the leader's currentTerm = the entry's term, 0 for NO_LEADER */
    int32_t status;    /* RAFT_PROPOSE_* */
} raft_ticket;
int raft_propose_batch    (raft_engine* e, const int64_t* group, const uint32_t* cmd, raft_ticket* ticket, int64_t n);
int raft_propose_batch_dev(raft_engine* e, const int64_t* group, const uint32_t* cmd, raft_ticket* ticket, int64_t n);

/* Resolve: what became of the entry ticket[m] names in group[m] (cmd[m]: the
 * command that was proposed).  Read-only; every record is filled.
 * - A group outside the engine: RAFT_TICKET_INVALID, counts 0.
 * - Else a ticket with status NO_LEADER or LOG_FULL: RAFT_TICKET_NONE, counts 0.
 * - Else a ticket with replica outside -1..R-1 or index outside
 *   0..log_cap-1: RAFT_TICKET_INVALID, counts 0.
 * - Else slot `index` of every replica of the group is looked up (holders,
 *   committed_on, unknown below; a replica counted in unknown is not read and
 *   is no holder) and the status is COMMITTED if
 *   committed_on >= 1, otherwise UNKNOWN if unknown >= 1, otherwise PENDING if
 *   the ticket's own replica is a holder, otherwise LOST.  A GHOSTED ticket
 *   gets no special case: it is looked up like any other and is normally LOST
 *   at once.
 * Returns RAFT_ERANGE if any group was out of range, otherwise RAFT_EINVAL if
 * any ticket had a bad replica or index (also: null engine, n < 0 or n >= 2^31,
 * a null buffer with n > 0, and then nothing is filled), otherwise
 * RAFT_EWINDOW if any record is UNKNOWN, otherwise RAFT_OK.
 * Not promised: in RAFT_MODE_REFERENCE a COMMITTED entry can later turn LOST
 * (quirks Q4 and Q9).  In RAFT_MODE_TEXTBOOK COMMITTED is final.
 * Ordering as the drain's; the _dev form takes DEVICE pointers (ticket and
 * out 16-byte aligned) and returns after its kernel finished. */
#define RAFT_TICKET_NONE      0  /* the ticket stored nothing (NO_LEADER, LOG_FULL) */
#define RAFT_TICKET_COMMITTED 1
#define RAFT_TICKET_PENDING   2
#define RAFT_TICKET_LOST      3
#define RAFT_TICKET_UNKNOWN   4  /* log_window only: the answer depends on a slot below a window */
#define RAFT_TICKET_INVALID   5  /* group, replica or index outside the engine: nothing was read */
typedef struct raft_ticket_state {  /* 16 bytes */
    int32_t status;
    int32_t holders;       /* replicas r with index < lastIndex_r and log_r[index] == (term, cmd) */
    int32_t committed_on;  /* holders with index < clamp(min(commitIndex_r, lastIndex_r), 0, log_cap) */
    int32_t unknown;       /* replicas whose slot `index` is below their window (index < physLen_r - W) */
} raft_ticket_state;
int raft_engine_resolve_tickets    (raft_engine* e, const int64_t* group, const raft_ticket* ticket, const uint32_t* cmd,
                                    raft_ticket_state* out, int64_t n);
int raft_engine_resolve_tickets_dev(raft_engine* e, const int64_t* group, const raft_ticket* ticket, const uint32_t* cmd,
                                    raft_ticket_state* out, int64_t n);

/* ---- the replicated state machine: committed entries applied on the device --
 * Additive to ABI 2 (RAFT_ABI_VERSION stays 2: nothing that existed changed).
 *
 * The step after "committed": a state machine per replica that consumes its
 * replica's committed entries in log order, in HBM, with no record written
 * per entry.  Opt-in: raft_engine_sm_configure(e, S) allocates it (S register
 * slots, a power of two in 1..64), and until then every other
 * raft_engine_sm_* call returns RAFT_EINVAL.  The canonical state, the
 * digest, the step kernel and the drain's lastApplied do not know about it.
 *
 * Per replica: reg[S] uint32 (0), hash uint64 (0), applied int32 (0: the
 * machine's own cursor, independent of the drain's lastApplied -- a caller may
 * drain to the host and apply on the device side by side) and lost int32 (0;
 * log_window only).  Applying entry (index i, term t, cmd c):
 *   reg[c & (S - 1)] = c                                    last writer wins
 *   hash = hash * 0xD1342543DE82EF95 + x(i, t, c)           mod 2^64
 *   x    = fmix((((uint64)(uint32)t << 32) | c) + (uint64)(uint32)i * 0x9E3779B97F4A7C15)
 *   fmix(z): z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31
 * Entries apply in ascending index.
 *
 * raft_engine_sm_apply visits the selected replicas of groups [g0, g0 + n) as
 * the drain does (replica = -1: every replica; else that replica index of each
 * group).  For each, with hi = clamp(min(commitIndex, lastIndex), 0, log_cap)
 * and lo = applied:
 * - with a log_window W and wl = max(0, physLen - W): if wl > lo and hi > lo,
 *   the min(wl, hi) - lo entries below the window are gone; they are added to
 *   the replica's `lost` and to info->lost, the cursor moves past them, and the
 *   call returns RAFT_EWINDOW after doing everything else;
 * - if hi < lo the replica is counted in info->regressed; nothing is applied
 *   and its cursor is unchanged;
 * - else entries lo .. hi - 1 are applied and applied = hi.
 * There is no max_entries: nothing is written per entry.
 *
 * Not promised, as with the drain: in RAFT_MODE_REFERENCE an applied entry may
 * later be overwritten in the log (quirks Q1-Q4, Q9); a replica's machine is
 * then not the fold of its current log, and a group's replicas may diverge.
 * In RAFT_MODE_TEXTBOOK with a flat log a replica's machine always equals the
 * fold of log[0, applied).
 *
 * Ordering is the drain's: the call runs on the engine stream, sees every step
 * enqueued before it, later step launches wait for it, and it returns when its
 * kernel has finished. */
typedef struct raft_sm_info {         /* 32 bytes */
    int64_t applied;     /* entries applied by this call */
    int64_t lost;        /* log_window only: entries that left the window unapplied; skipped */
    int64_t regressed;   /* selected replicas whose min(commit, last) < applied */
    int64_t reserved;    /* 0 */
} raft_sm_info;
typedef struct raft_sm_head {         /* 16 bytes */
    int32_t  applied;    /* entries [0, applied) of the replica's log were consumed (or skipped: lost) */
    int32_t  lost;       /* of those, the entries that were never applied */
    uint64_t hash;
} raft_sm_head;
typedef struct raft_sm_value {        /* 16 bytes */
    uint32_t value;      /* reg[key & (S - 1)] of the chosen replica, 0 if none */
    int32_t  replica;    /* the replica read: the one asked for, or the group's leader; -1 if it has none */
    int32_t  applied;    /* that replica's cursor ... */
    int32_t  commit;     /* ... and its commitIndex: how stale the answer is (0 if none) */
} raft_sm_value;
/* Allocate and zero the machine with `slots` registers per replica (again: zero
 * it, or reallocate for another count); slots = 0 frees it.  RAFT_EINVAL:
 * null engine, slots not 0 or a power of two in 1..64.  The allocation counts
 * in raft_engine_device_bytes, raft_engine_trim_staging keeps it, and
 * raft_engine_reset zeroes it. */
int raft_engine_sm_configure(raft_engine* e, int32_t slots);
/* RAFT_EINVAL: null engine or info, not configured, replica outside -1..R-1;
 * RAFT_ERANGE: groups outside the engine. */
int raft_engine_sm_apply(raft_engine* e, int64_t g0, int64_t n, int32_t replica, raft_sm_info* info);
/* The machines of groups [g0, g0 + n): heads [n][R], regs [n][R][S] (host;
 * either may be NULL).  sm_write resumes a run (with write_state / write_log):
 * every applied must be in 0..log_cap and every lost >= 0, else RAFT_EINVAL
 * and nothing is stored. */
int raft_engine_sm_read(raft_engine* e, int64_t g0, int64_t n, raft_sm_head* heads, uint32_t* regs);
int raft_engine_sm_write(raft_engine* e, int64_t g0, int64_t n, const raft_sm_head* heads, const uint32_t* regs);
/* The batched client read: out[m] = register key[m] of replica[m] of group[m]
 * (host arrays of n); replica[m] = -1 reads the group's leader as
 * raft_leader_info.leader chooses it.  A group outside the engine or a replica
 * outside -1..R-1 fails the whole batch with RAFT_ERANGE (nothing is filled).
 * n == 0 is RAFT_OK.  RAFT_EINVAL: null engine, not configured, n < 0 or
 * n >= 2^31, a null buffer with n > 0. */
int raft_engine_sm_get(raft_engine* e, const int64_t* group, const int32_t* replica, const uint32_t* key,
                       raft_sm_value* out, int64_t n);
/* State Machine Safety (the shape of raft_engine_check_log_matching): a group
 * of [g0, g0 + n) is flagged when two of its replicas have lost == 0, equal
 * applied and different hash.  *diverged = flagged groups; flags (nullable,
 * host, n bytes) receives 1 per flagged group.  An observation about the
 * protocol, never an engine error: RAFT_MODE_REFERENCE can flag groups
 * (quirks Q4, Q9), RAFT_MODE_TEXTBOOK must not. */
int raft_engine_sm_check(raft_engine* e, int64_t g0, int64_t n, uint8_t* flags, int64_t* diverged);

/* ---- replica crash and restart: volatile state lost on the device -----------
 * Additive to ABI 2 (RAFT_ABI_VERSION stays 2: nothing that existed changed).
 *
 * The reference's counterpart is killing a node's JVM and launching it again
 * (main, RaftServer.kt:302-310): it persists nothing, so the new process
 * starts from RaftServer.kt:35-48.  Here one kernel resets the chosen replicas
 * in HBM, between two step launches, without a copy of the state to the host,
 * and the caller says how much the process kept on disk.
 *
 * A restarted replica r, in terms of the canonical export (read_state):
 * - role = FOLLOWER, commitIndex = 0, phaseMs = retryMs = 0;
 * - flags = RAFT_FL_ARMED alone, what raft_engine_create leaves: no election,
 *   backoff, heartbeat session, pending-vote, votes or latch bits;
 * - rows next[r][*] and match[r][*] = 0, what raft_engine_create leaves;
 * - electionMs = a fresh timeout by the rule of a handler batch's timer reset:
 *   the replica's RAFT_RNG_TIMER word at the engine's current step index,
 *   scaled to election_min_ms..election_max_ms;
 * - flags 0: currentTerm, votedFor, lastIndex, physLen and the log are kept
 *   (the Raft paper's persistent state), and so are lastApplied and the
 *   machine: a durable consumer.  The drain and sm_apply then see
 *   min(commit, last) < cursor, count the replica in `regressed` and go on once
 *   its commitIndex has caught up;
 * - RAFT_RESTART_REPLAY: also lastApplied = 0 and, if a machine is configured,
 *   its head (applied, lost, hash) and registers = 0;
 * - RAFT_RESTART_AMNESIA: also currentTerm = 0, votedFor = -1, lastIndex =
 *   physLen = 0 (the row's slots are not cleared: slots at or beyond physLen are
 *   unspecified), and everything REPLAY does.
 * No other replica changes: the pending-vote bits others hold towards r stay.
 * The engine's own mirrors (the log-tail cache, the session rows' placement)
 * end up as a write_state of the same words would leave them, without the
 * engine-wide cache rebuild a write_state causes.
 *
 * Selection, over groups [g0, g0 + n):
 * - a mask of n bytes: bit r of mask[j] restarts replica r of group g0 + j
 *   (bits at or above R are ignored); host memory, or with _dev device memory
 *   under the buffer rules of raft_*_batch_dev;
 * - _random: replica r of global group id gid restarts when
 *   w < ceil(ppm * 2^32 / 10^6), w the RAFT_RNG_RESTART word of (step index,
 *   gid, r): 10^6 ppm selects every replica, 0 none.  Nothing is read from the
 *   host, and the same seed and step index select the same replicas.
 *
 * down_steps > 0 (at most 2^23 - 1): every group with a restarted replica gets
 * its isolation word (RAFT_GROUP_EXTRA[0]) set to down_steps << 8 | its lowest
 * restarted replica, over an isolation already running.  This is the harness's
 * isolation (churn_ppm), not a frozen process: for down_steps steps that replica
 * is cut off in both directions while its timers keep running, and at most one
 * replica per group can be down.  down_steps = 0 leaves the word alone.
 *
 * Not promised: RAFT_RESTART_AMNESIA forgets votes and log entries that other
 * replicas counted on, so RAFT_C_DUAL_LEADER_GROUPS, raft_engine_check_log_matching
 * and raft_engine_sm_check may report violations afterwards in either mode.
 *
 * Ordering is the drain's: the call runs on the engine stream, sees every step
 * enqueued before it, later step launches wait for it, and it returns when its
 * kernel has finished.
 * RAFT_EINVAL: null engine or info, a null mask with n > 0, unknown flag bits,
 * down_steps outside 0..2^23-1; RAFT_ERANGE: groups outside the engine.  n == 0
 * is RAFT_OK with a zeroed info. */
#define RAFT_RESTART_AMNESIA 1   /* also forget currentTerm, votedFor and the log (the reference persists nothing) */
#define RAFT_RESTART_REPLAY  2   /* also zero the consumers: lastApplied and, if configured, the machine
                                    (Raft Fig. 2: lastApplied is volatile; the log is replayed from 0) */
typedef struct raft_restart_info {  /* 32 bytes */
    int64_t restarted;        /* replicas restarted */
    int64_t leaders;          /* of those, the ones whose role was LEADER */
    int64_t entries_dropped;  /* AMNESIA: sum of their lastIndex before the call, else 0 */
    int64_t reserved;         /* 0 */
} raft_restart_info;
int raft_engine_restart       (raft_engine* e, int64_t g0, int64_t n, const uint8_t* mask_host,
                               int32_t flags, int32_t down_steps, raft_restart_info* info);
int raft_engine_restart_dev   (raft_engine* e, int64_t g0, int64_t n, const uint8_t* mask_dev,
                               int32_t flags, int32_t down_steps, raft_restart_info* info);
int raft_engine_restart_random(raft_engine* e, int64_t g0, int64_t n, uint32_t ppm,
                               int32_t flags, int32_t down_steps, raft_restart_info* info);

/* ---- linearizable reads: ReadIndex tickets confirmed on the device ----------
 * Additive to ABI 2 (RAFT_ABI_VERSION stays 2: nothing that existed changed).
 *
 * raft_engine_sm_get reads "the group's leader" as raft_leader_info.leader
 * chooses it and says how far that replica has applied.  That is a best-effort
 * read: an isolated leader keeps the role LEADER for many steps after the rest
 * of the group elected a successor in a higher term, it is often the lowest
 * id, and its applied == commit looks perfectly fresh; a freshly elected
 * leader's commitIndex can lag behind writes a client already saw COMMITTED.
 * The pair below is Raft's ReadIndex protocol (Ongaro's thesis §6.4), shaped
 * like propose / resolve: begin hands out a ticket (which leader, which term,
 * how far it had committed), serve confirms the ticket and reads.  Both calls
 * are read-only on the canonical state, the logs, the digest, lastApplied and
 * the machine.
 *
 * Begin: message m asks for a read index in group[m].
 * - The leader L is the replica with role LEADER that has the highest
 *   currentTerm, the lowest index among equals.  Not raft_leader_info.leader's
 *   rule: a deposed leader at a lower index must not shadow its successor.
 * - T = currentTerm_L and hi = clamp(min(commitIndex_L, lastIndex_L), 0,
 *   log_cap): the committed prefix the drain and sm_apply use.
 * - The ticket, first match wins:
 *     no replica is LEADER                         (-1, 0, -1, NO_LEADER)
 *     log_window only: hi > 0 and slot hi - 1 of L
 *       is below its window (hi - 1 < physLen_L - W)
 *       (hi == 0 names no slot: never UNKNOWN)     (L, T, hi, UNKNOWN); not read
 *     hi == 0 or log_L[hi - 1].term != T           (L, T, hi, TERM_UNCOMMITTED)
 *     otherwise                                    (L, T, hi, ISSUED)
 *   TERM_UNCOMMITTED: L has not yet committed an entry of its own term, so its
 *   commitIndex may lag behind acknowledged writes.  raft_engine_append_noops
 *   (below) gives such a leader an entry of its own term; once that commits,
 *   the client begins again.
 * - A group outside the engine fails the whole batch with RAFT_ERANGE before any
 *   ticket is written, as raft_propose_batch does.  n == 0 is RAFT_OK.  n < 2^31.
 *   RAFT_EWINDOW if any ticket is UNKNOWN, after filling every ticket.
 * - The machine need not be configured.
 *
 * Serve: out[m] = register key[m] of the replica ticket[m] names in group[m],
 * if the ticket still holds.  Needs raft_engine_sm_configure (else
 * RAFT_EINVAL, like every raft_engine_sm_* call).  Every record is filled;
 * first match wins:
 *   INVALID    group outside the engine, replica outside 0..R-1 or read_index
 *              outside 0..log_cap (a NO_LEADER ticket, with its -1s, included:
 *              serve what begin ISSUED); nothing is read
 *   NONE       the ticket's status is not ISSUED
 *   DEPOSED    the ticket's replica no longer has role LEADER with
 *              currentTerm == ticket.term; the client begins again
 *   NO_QUORUM  agree < R / 2 + 1, where agree counts the group's replicas (the
 *              ticket's included) whose currentTerm == ticket.term
 *   BEHIND     the replica's machine has applied < read_index; the caller runs
 *              raft_engine_sm_apply and serves again
 *   GAPPED     the machine's lost != 0: its registers are not the fold of the log
 *   SERVED     value = reg[key & (S - 1)] of that replica
 * agree is filled from DEPOSED on, applied (the replica's cursor) from BEHIND
 * on, value in SERVED; every other word is 0.
 * Returns RAFT_ERANGE if any group was out of range, otherwise RAFT_EINVAL if
 * any ticket had a bad replica or read_index (also: null engine, not
 * configured, n < 0 or n >= 2^31, a null buffer with n > 0, and then nothing is
 * filled), otherwise RAFT_OK.
 *
 * Why the quorum check is enough.  A leader of a term above T needs votes
 * from a majority whose terms are then above T; that majority would intersect
 * the majority found at exactly T.  So at the instant of the serve L is the
 * newest leader.  Once L has committed an entry of its own term (ISSUED), its
 * committed prefix at begin covered every write acknowledged before begin, and
 * the machine has applied at least that far.  The confirmation is the engine
 * reading the replicas' term words in HBM: a lossless, instantaneous
 * heartbeat round.  Drops, partitions and the isolation word are deliberately
 * not consulted: they decide how long an isolated leader can still serve,
 * never safety.
 *
 * Not promised: in RAFT_MODE_REFERENCE quirks Q4 and Q9 let committed entries
 * vanish, as the drain, the tickets and the machine already say, and
 * RAFT_RESTART_AMNESIA forgets votes and entries.  Promised in
 * RAFT_MODE_TEXTBOOK with a flat log and no amnesia.
 *
 * Ordering as the client path's: each call runs on the engine stream, sees
 * every step enqueued before it, later step launches wait for it, and it
 * returns when its kernel has finished.  The _dev forms take DEVICE pointers
 * under the buffer rules of raft_*_batch_dev; ticket and out must be 16-byte
 * aligned. */
#define RAFT_READ_ISSUED           0
#define RAFT_READ_TERM_UNCOMMITTED 1  /* the leader has committed no entry of its own term yet */
#define RAFT_READ_NO_LEADER        2  /* no replica of the group is LEADER */
#define RAFT_READ_UNKNOWN          3  /* log_window only: the slot that decides is below the leader's window */
typedef struct raft_read_ticket {     /* 16 bytes */
    int32_t replica;     /* the leader chosen, -1 for NO_LEADER */
    int32_t term;        /* its currentTerm, 0 for NO_LEADER */
    int32_t read_index;  /* its committed prefix: entries [0, read_index) must be applied before the read; -1 for NO_LEADER */
    int32_t status;      /* one of the four above */
} raft_read_ticket;
#define RAFT_READ_SERVED    0
#define RAFT_READ_BEHIND    1
#define RAFT_READ_GAPPED    2
#define RAFT_READ_NO_QUORUM 3
#define RAFT_READ_DEPOSED   4
#define RAFT_READ_NONE      5
#define RAFT_READ_INVALID   6
typedef struct raft_read_result {     /* 16 bytes */
    uint32_t value;
    int32_t  status;     /* one of the seven above */
    int32_t  applied;
    int32_t  agree;
} raft_read_result;
int raft_read_begin_batch    (raft_engine* e, const int64_t* group, raft_read_ticket* ticket, int64_t n);
int raft_read_begin_batch_dev(raft_engine* e, const int64_t* group, raft_read_ticket* ticket, int64_t n);
int raft_read_serve_batch    (raft_engine* e, const int64_t* group, const raft_read_ticket* ticket, const uint32_t* key,
                              raft_read_result* out, int64_t n);
int raft_read_serve_batch_dev(raft_engine* e, const int64_t* group, const raft_read_ticket* ticket, const uint32_t* key,
                              raft_read_result* out, int64_t n);

/* ---- snapshot install: a lagging replica healed from its leader on the device -
 * Additive to ABI 2 (RAFT_ABI_VERSION stays 2: nothing that existed changed).
 *
 * The reference has no counterpart: it has neither log compaction nor a
 * snapshot.  The source is the Raft paper's §7 (InstallSnapshot).  The
 * log_window ring already compacts physically; this is the other half, the way
 * back for a replica whose missing entries have left the leader's window (or,
 * on a flat log, one that would otherwise catch up one AppendEntries a step).
 * One kernel between two step launches copies the leader's retained log, its
 * machine and its commit point into the chosen replicas in HBM; nothing goes
 * through the host.  The snapshot IS the leader's machine, so the call needs
 * raft_engine_sm_configure.
 *
 * Per group of [g0, g0 + n):
 * - The leader L is chosen by the read path's rule (raft_read_begin_batch): the
 *   replica with role LEADER and the highest currentTerm, the lowest index
 *   among equals.  Not raft_leader_info.leader.  T = currentTerm_L and hi =
 *   clamp(min(commitIndex_L, lastIndex_L), 0, log_cap).
 * - No replica is LEADER: the group counts in no_leader.  L's machine has
 *   lost != 0 (it is not the fold of its log): the group counts in
 *   leader_gapped.  Neither kind of group is changed.  Both are counted
 *   whatever the mask says.
 * - Replica f is installed when it is eligible (bit f of mask[j] for group
 *   g0 + j; bits at or above R are ignored; a NULL mask makes every replica
 *   eligible), f != L, currentTerm_f <= T (an eligible f != L with a higher
 *   term counts in `ahead` and is skipped) and lastIndex_L - lastIndex_f >=
 *   min_lag (min_lag 0: every such replica, even one level with L).
 *
 * An installed f, in terms of read_state / read_log / sm_read, with floor =
 * max(0, physLen_L - log_window) on a ring and 0 on a flat log:
 * - lastIndex_f = lastIndex_L, physLen_f = physLen_L, and slots [floor,
 *   physLen_L) of f's row are copies of L's (slots_copied adds physLen_L -
 *   floor); its other slots are unspecified beyond what read_log zeroes;
 * - commitIndex_f = hi, currentTerm_f = T, votedFor_f kept if currentTerm_f was
 *   T already, else -1;
 * - the volatile state is what raft_engine_restart leaves: role FOLLOWER, flags
 *   RAFT_FL_ARMED alone, phaseMs = retryMs = 0, electionMs a fresh draw (the
 *   replica's RAFT_RNG_TIMER word at the engine's step index), rows next[f][*]
 *   and match[f][*] = 0;
 * - the leader's session towards it: next[L][f] = lastIndex_L + 1 and
 *   match[L][f] = lastIndex_L, what the leader holds after f acknowledged
 *   everything.  No other word of L changes;
 * - the machine: f's head (applied, lost, hash) and registers are copies of L's;
 * - lastApplied (the drain's cursor) is not touched: the drain's own lost /
 *   regressed rules cover it.
 * The engine's mirrors (the log-tail cache, the session rows' placement) end up
 * as a write_state + write_log + sm_write of the same words would leave them,
 * without the engine-wide cache rebuild.
 *
 * The call is the same in both protocol modes.  Promised in RAFT_MODE_TEXTBOOK
 * without RAFT_RESTART_AMNESIA: the install equals what a lossless run of
 * AppendEntries from L at term T would eventually produce, so
 * RAFT_C_DUAL_LEADER_GROUPS, raft_engine_check_log_matching and
 * raft_engine_sm_check stay clean.  In RAFT_MODE_REFERENCE it is defined but
 * nothing is promised (ghost tails, Q4, Q9), as elsewhere.  Drops, partitions
 * and the isolation word are not consulted: the install is a teleport, the same
 * lossless instantaneous round as the read path's confirmation.
 *
 * Ordering is raft_engine_restart's: the engine stream, later step launches
 * wait for it, it returns when its kernel has finished.  The _dev form takes
 * the mask in DEVICE memory under the buffer rules of raft_*_batch_dev.
 * RAFT_EINVAL: null engine or info, the machine not configured, min_lag < 0;
 * RAFT_ERANGE: groups outside the engine.  n == 0 is RAFT_OK with a zeroed info. */
typedef struct raft_install_info {   /* 64 bytes */
    int64_t installed;      /* replicas installed */
    int64_t slots_copied;   /* log slots copied into them */
    int64_t no_leader;      /* groups of the range with no LEADER: nothing done */
    int64_t leader_gapped;  /* groups whose leader's machine has lost != 0: nothing done */
    int64_t ahead;          /* masked replicas with currentTerm > the leader's: skipped */
    int64_t reserved[3];    /* 0 */
} raft_install_info;
int raft_engine_install_snapshot    (raft_engine* e, int64_t g0, int64_t n, const uint8_t* mask_host,
                                     int32_t min_lag, raft_install_info* info);
int raft_engine_install_snapshot_dev(raft_engine* e, int64_t g0, int64_t n, const uint8_t* mask_dev,
                                     int32_t min_lag, raft_install_info* info);

/* ---- leadership transfer: TimeoutNow on the device, with tickets -------------
 * Additive to ABI 2 (RAFT_ABI_VERSION stays 2: nothing that existed changed).
 *
 * The reference has no counterpart: its leader only ever loses leadership by
 * timeout.  The source is Ongaro's thesis §3.10 (TimeoutNow), as etcd and
 * hashicorp/raft ship it: before a planned restart (raft_engine_restart with
 * down_steps) a replica hands its groups on, instead of leaving each of them
 * leaderless for an election timeout.  A transfer is "the target's election
 * timer fires now": the only word a call writes is the target's electionMs = 1,
 * so phase T of the next step fires it, for any heartbeat period, and the
 * election runs under the step's own rules.  Nothing else is written, neither
 * on the leader nor in the sessions, and no engine-wide rebuild follows; the
 * word has no mirror in the engine, so the state is what a write_state of the
 * same word would leave.
 *
 * Transfer: message m asks group[m] to move its leadership to replica
 * target[m], or with RAFT_TRANSFER_AUTO to the best-placed other replica.
 * - `from` is the group's newest leader by the read path's rule
 *   (raft_read_begin_batch): role LEADER, the highest currentTerm, the lowest
 *   index among equals.
 * - The ticket's status, first match wins:
 *     INVALID      target outside -1..R-1: nothing was read or written  (-1, 0, -1)
 *     NO_LEADER    no replica of the group is LEADER                     (-1, 0, -1)
 *     SELF         target == from: nothing to do                         (from, T, -1)
 *     BEHIND       the target's (lastIndex, last log term) differ from
 *                  the leader's: the thesis's "caught up", read from HBM
 *                  as the read path reads its heartbeat round (lossless
 *                  and instantaneous), not from matchIndex               (from, T, -1)
 *     BUSY         the target's role is not FOLLOWER, or its flags lack
 *                  RAFT_FL_ARMED, or have RAFT_FL_ELECTING, RAFT_FL_BACKOFF
 *                  or RAFT_FL_PENDING_RST (electing, a candidate, a stale
 *                  leader of a lower term)                               (from, T, -1)
 *     UNREACHABLE  the group's isolation word (RAFT_GROUP_EXTRA[0]) has
 *                  steps left and names the target                       (from, T, -1)
 *     SENT         the target's electionMs = 1                           (from, T, target)
 *   With RAFT_TRANSFER_AUTO the replicas other than `from` are judged by the
 *   same three rules in the order from + 1, from + 2, ... (mod R) and the first
 *   that passes is the target: "caught up" already makes every candidate's log
 *   the leader's, and the cyclic order spreads leaders instead of piling them
 *   on replica 0.  None passes (always so at R = 1): NO_TARGET (from, T, -1).
 * - Several messages for one group are each judged against the state before
 *   the call and honoured on their own: the same target twice is idempotent,
 *   two different targets fire two timers and the step's election decides.
 * - A group outside the engine fails the whole batch with RAFT_ERANGE before
 *   anything is written, as raft_read_begin_batch does.  n == 0 is RAFT_OK.
 *   n < 2^31.  RAFT_EINVAL: null engine, n < 0, a null buffer with n > 0.
 * - It reads no log slot, so every log layout is served alike; the last log
 *   term is the engine's log-tail cache, rebuilt first where a write_state /
 *   write_log left it stale, as the handler batches do.
 *
 * Resolve: what became of ticket[m] of group[m].  Every record is filled; first
 * match wins:
 *   INVALID     the group is outside the engine, or a SENT ticket's from or
 *               target is outside 0..R-1; nothing is read          (leader -1, term 0)
 *   NONE        the ticket's status is not SENT                    (leader -1, term 0)
 *   COMPLETED   the target is LEADER in a term above the ticket's  (target, its term)
 *   SUPERSEDED  another replica is: the newest of them             (that replica, its term)
 *   PENDING     no replica is LEADER in a term above the ticket's  (leader -1, term 0)
 * Read-only.  Returns RAFT_ERANGE if any group was out of range, otherwise
 * RAFT_EINVAL if any SENT ticket had a bad from or target (also: null engine,
 * n < 0 or n >= 2^31, a null buffer with n > 0, and then nothing is filled),
 * otherwise RAFT_OK.
 *
 * Evacuate, the range form for a planned restart: for each group of [g0, g0 + n)
 * whose newest leader `from` has its bit set in mask[j] (the layout of
 * raft_engine_restart's mask; bits at or above R are ignored), the AUTO rule
 * with the masked replicas excluded as targets.  Groups led from outside the
 * mask, and groups without a leader, are untouched.  There is no ticket (a
 * caller that wants tickets uses the batch form); the info counts groups:
 * `led` from inside the mask, of those `sent` and `no_target` (led = sent +
 * no_target), and of the no_target groups `behind`, those with an unmasked
 * replica refused as BEHIND, and `busy`, those with one refused as BUSY or
 * UNREACHABLE (a group may count in both, or in neither when every other
 * replica is masked).
 * RAFT_EINVAL: null engine or info, a null mask with n > 0; RAFT_ERANGE: groups
 * outside the engine.  n == 0 is RAFT_OK with a zeroed info.
 *
 * Both protocol modes.  In RAFT_MODE_REFERENCE the effect is whatever the
 * reference does when that timer fires.  Promised in RAFT_MODE_TEXTBOOK with a
 * flat log and no RAFT_RESTART_AMNESIA: a transfer is a timeout, which Raft
 * tolerates at any moment, so Election Safety is untouched --
 * RAFT_C_DUAL_LEADER_GROUPS, raft_engine_check_log_matching and
 * raft_engine_sm_check stay at 0.  Not promised: that the target wins.  The old
 * leader goes on accepting proposals until it hears of the new term; one that
 * lands between the call and the next step makes the target's log shorter than
 * the leader's, and its win then depends on the other followers' logs.  That is
 * safe; the ticket says PENDING or SUPERSEDED and the caller transfers again.
 *
 * Ordering is raft_engine_restart's: each call runs on the engine stream, sees
 * every step enqueued before it, later step launches wait for it, and it
 * returns when its kernel has finished.  The _dev forms take DEVICE pointers
 * under the buffer rules of raft_*_batch_dev; ticket and out must be 16-byte
 * aligned. */
#define RAFT_TRANSFER_AUTO       (-1)  /* target: the best-placed other replica (rule above) */
#define RAFT_TRANSFER_SENT        0  /* the target's timer was set to fire in the next step */
#define RAFT_TRANSFER_NO_LEADER   1  /* no replica of the group is LEADER */
#define RAFT_TRANSFER_SELF        2  /* the target already is the group's newest leader: nothing to do */
#define RAFT_TRANSFER_BEHIND      3  /* the target's log is not the leader's (last index or last term differ) */
#define RAFT_TRANSFER_BUSY        4  /* the target is not an idle, armed FOLLOWER (electing, candidate, a stale leader) */
#define RAFT_TRANSFER_UNREACHABLE 5  /* the group's isolation word is running and names the target */
#define RAFT_TRANSFER_NO_TARGET   6  /* AUTO / evacuate: no replica qualifies */
#define RAFT_TRANSFER_INVALID     7  /* target outside -1..R-1: nothing was read or written */
typedef struct raft_transfer_ticket {  /* 16 bytes */
    int32_t from;     /* the leader the transfer left (-1: none) */
    int32_t term;     /* its term at the call */
    int32_t target;   /* the replica whose timer was set (AUTO resolved; -1: none) */
    int32_t status;   /* RAFT_TRANSFER_SENT ... RAFT_TRANSFER_INVALID */
} raft_transfer_ticket;
int raft_transfer_batch    (raft_engine* e, const int64_t* group, const int32_t* target, raft_transfer_ticket* ticket,
                            int64_t n);
int raft_transfer_batch_dev(raft_engine* e, const int64_t* group, const int32_t* target, raft_transfer_ticket* ticket,
                            int64_t n);
#define RAFT_TRANSFER_COMPLETED  0  /* the target is LEADER in a term above the ticket's */
#define RAFT_TRANSFER_PENDING    1  /* no replica is LEADER in a term above the ticket's */
#define RAFT_TRANSFER_SUPERSEDED 2  /* another replica is */
#define RAFT_TRANSFER_NONE       3  /* the ticket's status was not SENT */
/* RAFT_TRANSFER_INVALID as above: group, from or target outside the engine */
typedef struct raft_transfer_state {   /* 16 bytes */
    int32_t status;   /* one of the five above */
    int32_t leader;   /* COMPLETED / SUPERSEDED: the LEADER found, else -1 */
    int32_t term;     /* its term, else 0 */
    int32_t reserved; /* 0 */
} raft_transfer_state;
int raft_engine_resolve_transfers    (raft_engine* e, const int64_t* group, const raft_transfer_ticket* ticket,
                                      raft_transfer_state* out, int64_t n);
int raft_engine_resolve_transfers_dev(raft_engine* e, const int64_t* group, const raft_transfer_ticket* ticket,
                                      raft_transfer_state* out, int64_t n);
typedef struct raft_evacuate_info {    /* 64 bytes */
    int64_t led;          /* groups of the range whose newest leader is in the mask */
    int64_t sent;         /* of those, the groups in which a timer was set */
    int64_t no_target;    /* of those, the groups in which no replica qualified */
    int64_t behind;       /* of no_target, the groups with an unmasked replica refused as BEHIND */
    int64_t busy;         /* of no_target, the groups with one refused as BUSY or UNREACHABLE */
    int64_t reserved[3];  /* 0 */
} raft_evacuate_info;
int raft_engine_evacuate    (raft_engine* e, int64_t g0, int64_t n, const uint8_t* mask_host, raft_evacuate_info* info);
int raft_engine_evacuate_dev(raft_engine* e, int64_t g0, int64_t n, const uint8_t* mask_dev, raft_evacuate_info* info);

/* ---- leader no-op entries: commit and read liveness after an election --------
 * Additive to ABI 2 (RAFT_ABI_VERSION stays 2: nothing that existed changed).
 *
 * The reference has no counterpart.  The source is Ongaro's thesis §3.6.2 and
 * §6.4 step 1: a new leader appends an entry of its own term.  Without one, in
 * RAFT_MODE_TEXTBOOK (whose commit rule counts current-term entries only) the
 * entries of earlier terms stay uncommitted after a leader change until some
 * client proposes again: an idle group answers raft_read_begin_batch with
 * TERM_UNCOMMITTED for ever, and a raft_propose_batch ticket whose entry was
 * replicated but not committed before a restart, a partition, a
 * raft_transfer_batch or a raft_engine_evacuate stays PENDING.
 *
 * The call visits every group of [g0, g0 + n); nothing but the scalars comes
 * from the host.  Per group:
 * - L is the group's newest leader by the read path's rule
 *   (raft_read_begin_batch): role LEADER, the highest currentTerm, the lowest
 *   index among equals.  T = currentTerm_L.
 * - The group's record, first match wins:
 *     no replica is LEADER                       ticket (-1, -1, 0, NO_LEADER), ticket_cmd 0
 *     lastIndex_L >= 1 and the term of L's last  nothing is appended: ticket (L, lastIndex_L - 1,
 *       entry is T                                 T, CURRENT) names that entry, ticket_cmd its cmd
 *     otherwise                                  appendCommand of `cmd` on L: the ticket and status
 *                                                  raft_propose_batch writes for one message to L
 *                                                  (ACCEPTED, reference mode's GHOSTED, LOG_FULL),
 *                                                  ticket_cmd = cmd
 *   So a second call in the same term appends nothing -- but for reference
 *   mode's GHOSTED: that entry went to the physical end, the leader's visible
 *   tail is still the stale slot, and the next call judges by it.
 * - The effect on state, logs and the log-tail cache is exactly that of
 *   raft_append_command_batch called with (group, L, cmd) on the groups that
 *   appended; nothing else changes.  No log slot is read: the term of the last
 *   entry is the engine's log-tail cache, rebuilt first where a write_state /
 *   write_log left it stale, so every log layout is served alike.
 * - ticket and ticket_cmd ([n] each, the record of group g0 + j at j) are both
 *   given or both NULL.  (group, ticket, ticket_cmd) go to
 *   raft_engine_resolve_tickets unchanged: it treats CURRENT like every status
 *   other than NO_LEADER and LOG_FULL, as "stored".  COMMITTED there means "this
 *   leader has committed an entry of its own term", which is exactly
 *   raft_read_begin_batch's condition for ISSUED.
 * - info counts groups: appended (lastIndex_L grew: ACCEPTED or GHOSTED), of
 *   those ghosted, and current, no_leader, log_full; n = appended + current +
 *   no_leader + log_full.
 * - With a log_window, a RAFT_MODE_TEXTBOOK add below its replica's window
 *   returns RAFT_EWINDOW after doing everything, as raft_propose_batch does.
 * RAFT_EINVAL: null engine or info, only one of ticket and ticket_cmd, a _dev
 * ticket buffer that is not 16-byte aligned; RAFT_ERANGE: groups outside the
 * engine.  n == 0 is RAFT_OK with a zeroed info.
 *
 * The entry is an ordinary entry: the drain delivers it, and the caller knows
 * the id it chose.  A state machine passes over it after
 * raft_engine_sm_set_noop: while enabled, raft_engine_sm_apply treats an entry
 * whose cmd equals `cmd` like any other for applied, lost and hash and writes
 * no register for it.  Disabled is the default.  The setting is the engine's,
 * not the machine's data: it may be set before raft_engine_sm_configure, and
 * raft_engine_reset, sm_configure, sm_write, restart and snapshot install leave
 * it alone.  RAFT_EINVAL: null engine.
 *
 * Both protocol modes.  Promised in RAFT_MODE_TEXTBOOK without
 * RAFT_RESTART_AMNESIA: the call is a client command, which Raft tolerates at
 * any moment, so RAFT_C_DUAL_LEADER_GROUPS, raft_engine_check_log_matching and
 * raft_engine_sm_check stay at 0.
 *
 * Ordering is raft_engine_restart's: the call runs on the engine stream, sees
 * every step enqueued before it, later step launches wait for it, and it
 * returns when its kernel has finished.  The _dev form takes DEVICE pointers
 * for the two arrays under the buffer rules of raft_*_batch_dev. */
#define RAFT_PROPOSE_CURRENT   4  /* raft_engine_append_noops: nothing appended, the leader's last entry is
                                     already of its own term; the ticket names that entry */
typedef struct raft_noop_info {   /* 64 bytes */
    int64_t appended;     /* groups whose leader got the entry (ACCEPTED or GHOSTED) */
    int64_t current;      /* groups whose leader's last entry was of its own term already */
    int64_t no_leader;    /* groups without a LEADER */
    int64_t log_full;     /* groups whose leader's Log.add was refused for lack of capacity */
    int64_t ghosted;      /* of appended, reference mode's GHOSTED */
    int64_t reserved[3];  /* 0 */
} raft_noop_info;
int raft_engine_append_noops    (raft_engine* e, int64_t g0, int64_t n, uint32_t cmd, raft_ticket* ticket_host,
                                 uint32_t* ticket_cmd_host, raft_noop_info* info);
int raft_engine_append_noops_dev(raft_engine* e, int64_t g0, int64_t n, uint32_t cmd, raft_ticket* ticket_dev,
                                 uint32_t* ticket_cmd_dev, raft_noop_info* info);
int raft_engine_sm_set_noop(raft_engine* e, int enable, uint32_t cmd);

/* ---- the leader watch: leadership changes as a delta stream ------------------
 * Additive to ABI 2 (RAFT_ABI_VERSION stays 2: nothing that existed changed).
 *
 * raft_engine_read_leaders returns 16 bytes for every group on every call and
 * names the lowest-id LEADER, after an isolation often a deposed one.  A
 * service that routes proposals and reads keeps a leader directory and needs
 * only the changes (etcd's SoftState in a Ready, TiKV's role observer): a poll
 * returns one record per group whose leader or term changed since the watch
 * last reported that group.  The reference has no counterpart.
 *
 * - The engine keeps one `seen` pair (leader, term) per group, 8 bytes, in an
 *   array of its own, as it does for lastApplied: it is not part of read_state
 *   / write_state or of the digest, and the step kernel and every other call
 *   never touch it.  It is allocated and set to (-1, 0) at the first call of
 *   this section that needs it, raft_engine_reset sets it back to (-1, 0), it
 *   counts in raft_engine_device_bytes and raft_engine_trim_staging keeps it.
 * - A group's current leader is its newest leader by raft_read_begin_batch's
 *   rule: role LEADER, the highest currentTerm, the lowest index among equals,
 *   with that replica's currentTerm; (-1, 0) when no replica is LEADER.
 *   Deliberately not raft_leader_info.leader: a deposed leader at a lower index
 *   must not shadow its successor in a routing table.
 * - A group of [g0, g0 + n) is changed when its current (leader, term) differs
 *   from `seen` in either word.  Its record carries both pairs.  The four kinds
 *   partition the changed groups: gained (prev_leader == -1, leader >= 0), lost
 *   (prev_leader >= 0, leader == -1), moved (both >= 0, different replicas),
 *   reterm (the same replica, another term).
 * - Records come in ascending group order, identical from run to run.  When
 *   more groups changed than max_events, exactly the first max_events of that
 *   order are written, `seen` advances only for the groups that were written
 *   and `pending` counts the rest: with no step in between, successive polls
 *   concatenated equal one poll with enough room.  The kind counts and
 *   `leaderless` describe the whole range at the call, not only what was
 *   delivered.  out == NULL with max_events == 0 is a peek: nothing is stored,
 *   not even `seen`.
 * RAFT_EINVAL: null engine or info, max_events < 0, out == NULL with
 * max_events > 0, a _dev buffer that is not 8-byte aligned; RAFT_ERANGE:
 * groups outside the engine.  n == 0 is RAFT_OK with a zeroed info.
 *
 * Both protocol modes and every log layout: no log slot is read.  Nothing about
 * Raft safety is promised or needed; the call reports role words.
 *
 * Ordering is raft_engine_drain_committed's: the call runs on the engine
 * stream, sees every step enqueued before it, and later step launches wait for
 * it.  The host variant returns after the copy; the _dev variant (out: a DEVICE
 * pointer to max_events records; info stays a host pointer) returns after its
 * kernels finished. */
typedef struct raft_leader_event {   /* 24 bytes */
    int64_t group;        /* engine-local group index */
    int32_t leader;       /* the group's newest leader now, -1 if none */
    int32_t term;         /* its currentTerm, 0 if none */
    int32_t prev_leader;  /* what the watch last reported for the group (-1, 0 before the first report) */
    int32_t prev_term;
} raft_leader_event;
typedef struct raft_watch_info {     /* 64 bytes */
    int64_t delivered;    /* events written to out */
    int64_t pending;      /* changed groups left for lack of room (all of them, in a peek) */
    int64_t gained;       /* of the changed groups (delivered + pending): prev_leader == -1, leader >= 0 */
    int64_t lost;         /*   prev_leader >= 0, leader == -1 */
    int64_t moved;        /*   both >= 0 and different replicas */
    int64_t reterm;       /*   the same replica, another term */
    int64_t leaderless;   /* groups of the range with no LEADER now, changed or not */
    int64_t reserved;     /* 0 */
} raft_watch_info;
int raft_engine_poll_leaders    (raft_engine* e, int64_t g0, int64_t n, raft_leader_event* out_host,
                                 int64_t max_events, raft_watch_info* info);
int raft_engine_poll_leaders_dev(raft_engine* e, int64_t g0, int64_t n, raft_leader_event* out_dev,
                                 int64_t max_events, raft_watch_info* info);
/* `seen` of groups [g0, g0 + n): [n][2] int32 (leader, term).  write_watch
 * resumes a consumer: every leader in -1..R-1 and every term >= 0, a leader of
 * -1 with term 0 only; anything else is RAFT_EINVAL and nothing is stored. */
int raft_engine_read_watch (raft_engine* e, int64_t g0, int64_t n, int32_t* out);
int raft_engine_write_watch(raft_engine* e, int64_t g0, int64_t n, const int32_t* in);

/* ---- the proposal outbox: retry lost proposals on the device, commit once -----
 * Additive to ABI 2 (RAFT_ABI_VERSION stays 2: nothing that existed changed).
 *
 * raft_propose_batch hands out a ticket and raft_engine_resolve_tickets says
 * what became of it; what a client does with a proposal that did not commit
 * (Raft thesis §6.3: "the client retries") is left to the caller.  The outbox
 * is that piece: a queue in HBM, opt-in per engine, that holds proposals until
 * they are committed, re-proposes exactly the ones that are provably gone and
 * hands completions out as a stream.  The step kernel, the canonical state and
 * the digest do not know about it; an engine that never configures one behaves
 * as before, byte for byte.  The reference has no counterpart (its /cmd route
 * forgets the command at once).
 *
 * Why "retry whatever resolved LOST" is wrong.  RAFT_TICKET_LOST says that the
 * ticket's own replica no longer holds the entry, nothing about the others.
 * Leader A appends (i, T, c) and replicates it to B; A's slot i is overwritten
 * by a short-lived leader of term T+1 whose entry reached A only; the ticket
 * resolves LOST with holders = 1.  B can still win term T+2 on the votes of
 * replicas that never saw the T+1 entry and commit (i, T, c): a client that
 * re-proposed c has committed it twice.  Only holders == 0 is final: no replica
 * has the entry, the engine has no message in flight between two steps, so
 * nothing can bring it back.
 *
 * A record (raft_outbox_entry, 48 bytes, the export form) is a proposal (group,
 * cmd) under the caller's tag, the step index at its submit (born), its current
 * raft_ticket (replica, index, term, status; (-1, -1, 0, RAFT_OUTBOX_NEW)
 * before the first proposal) and the number of times it was proposed (tries).
 *
 * raft_engine_outbox_configure(capacity, expire_steps): capacity >= 1 records,
 *   expire_steps >= 0 (0: never); anything else is RAFT_EINVAL.  Allocates the
 *   queue (2 x capacity x 48 bytes: a pump writes the survivors into the other
 *   half), which counts in raft_engine_device_bytes from then on and which
 *   raft_engine_trim_staging keeps (it frees the outbox's scratch).  The queue
 *   shares its allocation with the leader watch's `seen` pairs, which are
 *   allocated with it (8 bytes per group) if no call has needed them yet and
 *   keep their contents otherwise.  An empty outbox may be configured again; a
 *   non-empty one is RAFT_EINVAL.  raft_engine_reset empties the outbox and
 *   keeps its configuration.
 * raft_outbox_submit(group, cmd, tag, n): appends n records at the tail in
 *   batch order with status NEW, tries 0, born = raft_engine_step_index now.
 *   It proposes nothing.  RAFT_EINVAL: not configured, null array with n > 0,
 *   n < 0; RAFT_EFULL: n exceeds the free room; RAFT_ERANGE: a group outside
 *   the engine.  In each case nothing is enqueued.  n == 0 is RAFT_OK.
 * raft_engine_outbox_pump(done, max_done, n_done, info): two phases, on the
 *   state the call finds.
 *   Phase 1 gives every record a verdict from raft_engine_resolve_tickets'
 *   record of its ticket (a ticket of status NEW, NO_LEADER or LOG_FULL stored
 *   nothing: RAFT_TICKET_NONE); phase 2 changes no verdict.  With age = the
 *   step index now - born, the first match of:
 *     1. COMMITTED                               -> done, RAFT_OUTBOX_COMMITTED
 *     2. expire_steps > 0 and age >= expire_steps -> done, RAFT_OUTBOX_EXPIRED:
 *        the outcome is unknown, as after any client timeout (the entry may
 *        still commit later)
 *     3. UNKNOWN                                 -> kept (info.unknown)
 *     4. PENDING                                 -> kept (info.pending)
 *     5. LOST with holders >= 1                  -> kept (info.orphaned)
 *     6. LOST with holders == 0, or NONE         -> retried (info.retried)
 *   Phase 2: the first max_done done records in queue order are written to
 *   done[] in that order and leave the queue; the done records past the cut
 *   stay unchanged (info.deferred).  The retried records are proposed, in queue
 *   order, with exactly the effect of one raft_propose_batch over their
 *   (group, cmd): the same leader rule, the k-th accepted message to a group
 *   gets lastIndex + k, the same RAFT_EWINDOW rule.  Each one's ticket is
 *   replaced by the new one and its tries grow by 1 (a NO_LEADER or LOG_FULL
 *   ticket keeps the record for the next pump).  The queue becomes the surviving
 *   records in their original order.
 *   *n_done = records written (<= max_done).  RAFT_EINVAL: not configured, null
 *   n_done or info, max_done < 0, done == NULL with max_done > 0, a _dev buffer
 *   that is not 16-byte aligned.  Otherwise RAFT_EWINDOW when info.unknown > 0
 *   or a retried add was below its replica's window, after doing everything;
 *   otherwise RAFT_OK.
 *   info: queued = the queue's length at the call = committed + expired +
 *   deferred + pending + orphaned + unknown + retried; committed / expired
 *   count the records written to done[]; accepted + ghosted + no_leader +
 *   log_full = retried, by the status of the new tickets; left = the queue's
 *   length afterwards = queued - committed - expired.  age_hist counts the
 *   COMMITTED records this call wrote, in bucket min(31, floor(log2(age + 1))).
 * raft_engine_outbox_read(out, room, n): the queue in order, *n records.  out ==
 *   NULL with room 0 is a peek: RAFT_OK with *n = the queue's length; otherwise
 *   a room below the length is RAFT_EINVAL, with *n = the length and nothing
 *   copied.  raft_engine_outbox_write(in, n): replaces the queue.
 *   Refused before anything is stored: n above the capacity (RAFT_EFULL), a
 *   group outside the engine (RAFT_ERANGE), a status that is none of
 *   RAFT_OUTBOX_NEW / RAFT_PROPOSE_*, a ticket that stored an entry (ACCEPTED,
 *   GHOSTED, CURRENT) with a replica outside -1..R-1 or an index outside
 *   0..log_cap-1, tries < 0, a nonzero pad (RAFT_EINVAL).
 *
 * Promised: in RAFT_MODE_TEXTBOOK without RAFT_RESTART_AMNESIA no record's
 * command is ever committed under two different (index, term) -- provided the
 * caller submits each command once and proposes it through the outbox only.
 * Not promised: anything in reference mode (quirks Q1, Q4, Q9 lose and
 * duplicate entries on their own; the calls are defined and deterministic all
 * the same); progress in an idle group, which needs an entry of the current
 * term to commit older ones (raft_engine_append_noops).
 *
 * Ordering is raft_engine_drain_committed's: the calls run on the engine
 * stream, see every step enqueued before them, and later step launches wait
 * for them.  The _dev variants take DEVICE pointers for the arrays (n_done and
 * info stay host pointers) and return after their kernels finished. */
#define RAFT_OUTBOX_NEW       (-1)  /* raft_outbox_entry.status before the first proposal */
#define RAFT_OUTBOX_COMMITTED  1    /* raft_outbox_done.status */
#define RAFT_OUTBOX_EXPIRED    2
typedef struct raft_outbox_entry {   /* 48 bytes */
    int64_t  tag;        /* the caller's */
    int64_t  born;       /* raft_engine_step_index at the submit */
    int32_t  group;      /* engine-local */
    uint32_t cmd;
    int32_t  replica, index, term, status;   /* the record's raft_ticket; status RAFT_OUTBOX_NEW or RAFT_PROPOSE_* */
    int32_t  tries;      /* proposals made for it so far */
    int32_t  pad;        /* 0 */
} raft_outbox_entry;
typedef struct raft_outbox_done {    /* 32 bytes */
    int64_t tag;
    int32_t group;
    int32_t status;      /* RAFT_OUTBOX_COMMITTED / RAFT_OUTBOX_EXPIRED */
    int32_t index, term; /* of the record's last ticket: where it committed (COMMITTED) */
    int32_t tries;
    int32_t age;         /* the step index at this pump - born, clipped to int32 */
} raft_outbox_done;
typedef struct raft_outbox_info {    /* 360 bytes, all int64 */
    int64_t queued, committed, expired, deferred, pending, orphaned, unknown, retried;
    int64_t accepted, ghosted, no_leader, log_full, left;
    int64_t age_hist[32];
} raft_outbox_info;
int raft_engine_outbox_configure(raft_engine* e, int64_t capacity, int32_t expire_steps);
int raft_outbox_submit    (raft_engine* e, const int64_t* group, const uint32_t* cmd, const int64_t* tag, int64_t n);
int raft_outbox_submit_dev(raft_engine* e, const int64_t* group_dev, const uint32_t* cmd_dev, const int64_t* tag_dev,
                           int64_t n);
int raft_engine_outbox_pump    (raft_engine* e, raft_outbox_done* done_host, int64_t max_done, int64_t* n_done,
                                raft_outbox_info* info);
int raft_engine_outbox_pump_dev(raft_engine* e, raft_outbox_done* done_dev, int64_t max_done, int64_t* n_done,
                                raft_outbox_info* info);
int raft_engine_outbox_read (raft_engine* e, raft_outbox_entry* out, int64_t room, int64_t* n);
int raft_engine_outbox_write(raft_engine* e, const raft_outbox_entry* in, int64_t n);

/* ---- the safety audit: Raft invariants checked over time on the device --------
 * Additive to ABI 2 (RAFT_ABI_VERSION stays 2: nothing that existed changed).
 *
 * RAFT_C_DUAL_LEADER_GROUPS, raft_engine_check_log_matching and
 * raft_engine_sm_check look at the present instant and remember nothing: none
 * can see a committed entry that later changed or vanished, a later leader
 * that lacks a committed entry, a replica that voted twice in a term or a term
 * that went backwards (what RAFT_RESTART_AMNESIA does).  An audit is a ledger
 * per group that remembers what the group has shown, and raft_audit_observe
 * checks the state now against it.  The reference has no counterpart.
 *
 * - A raft_audit belongs to one engine and owns its HBM (raft_audit_device_bytes;
 *   raft_engine_device_bytes does not count it).  The engine does not know
 *   about it: the step kernel, the canonical state, the digest and every other
 *   call are as before, raft_engine_reset does NOT reach it (call
 *   raft_audit_reset), and it is destroyed before its engine.  observe and
 *   report never write engine memory.
 * - The ledger of one group, 8 + 2 R int32 words as raft_audit_read returns it:
 *     [0] flags             sticky RAFT_AUDIT_* bits                         0
 *     [1] first_step        raft_engine_step_index (low 32 bits) at the
 *                           observe where flags first left 0                 0
 *     [2] lead_term         the highest term in which a LEADER was observed  0
 *     [3] lead_replica      and who                                          -1
 *     [4] anchor_count  C   the longest committed prefix any replica showed  0
 *     [5] anchor_term       the entry at index C - 1 when C was recorded     0
 *     [6] anchor_cmd                                                         0
 *     [7] anchor_seen_term  the highest currentTerm in the group at the
 *                           observe that recorded C                          0
 *     [8 + 2r], [9 + 2r]    replica r's currentTerm, votedFor as last
 *                           observed                                         0, -1
 *   (last column: the zero state of create and reset).
 * - One observe of one group, in this order; "old" is the ledger before the
 *   call, hi_r = min(commitIndex_r, lastIndex_r) within 0..log_cap:
 *   1. per replica r: term_r < old term -> TERM_REGRESSED; term_r == old term,
 *      old votedFor >= 0 and voted_r != old votedFor -> VOTE_CHANGED; then the
 *      pair is stored.
 *   2. two replicas LEADER now with equal terms -> TWO_LEADERS; a replica r
 *      LEADER now with term_r == old lead_term, old lead_replica >= 0 and
 *      r != old lead_replica -> TWO_LEADERS; then the newest leader
 *      (raft_read_begin_batch's rule) is stored if its term > old lead_term.
 *   3. when old C > 0, with i = C - 1: every replica with hi_r >= C must hold
 *      (anchor_term, anchor_cmd) at i, else COMMIT_CHANGED (State Machine
 *      Safety over time); every replica LEADER now with term_r > old
 *      anchor_seen_term must have lastIndex_r >= C and hold the anchor at i,
 *      else LEADER_INCOMPLETE (Leader Completeness).  The term guard makes
 *      that sound: the anchor was committed in a term <= anchor_seen_term, and
 *      a stale leader of a lower term, still LEADER while isolated, may lack
 *      it (Figure 8 of the Raft paper).  With a log_window a slot below a
 *      replica's window (i < physLen_r - W) is not read: that check is skipped
 *      and counted in `unknown`, once per skipped check.
 *   4. C' = max_r hi_r.  If C' > C, the lowest r with hi_r == C' gives the new
 *      anchor (C', its entry at C' - 1) and anchor_seen_term = max_r term_r;
 *      if that slot is below its window, one `unknown` and the old anchor
 *      stays.  A smaller C' is normal (a restart sets commitIndex to 0, quirk
 *      Q4 lowers it) and raises nothing.
 *   5. the bits raised are OR-ed into flags; first_step is stored when flags
 *      leaves 0.
 * - raft_audit_report lists the groups of the range with flags != 0 in
 *   ascending group order, cut at max_events; `pending` counts the rest.  It
 *   consumes nothing: the same call returns the same records.  max_events == 0
 *   (with or without a buffer) is a peek.
 * - raft_audit_write resumes a ledger.  RAFT_EINVAL with nothing stored:
 *   unknown flag bits, lead_replica outside -1..R-1, anchor_count outside
 *   0..log_cap.  No other word is ever used as an index.
 * RAFT_EINVAL: null handle or info, max_events < 0, out == NULL with
 * max_events > 0, a _dev buffer that is not 16-byte aligned; RAFT_ERANGE:
 * groups outside the engine.  n == 0 is RAFT_OK with a zeroed info.
 *
 * Both protocol modes and every log layout.  Promised: in RAFT_MODE_TEXTBOOK
 * on persistent logs (no RAFT_RESTART_AMNESIA) no flag is ever raised, whatever
 * the faults, restarts, installs, transfers, no-ops and outbox traffic and
 * however rarely observe is called.  In reference mode and after an amnesia
 * restart the flags are observations about the protocol, as with
 * raft_engine_check_log_matching.  The rules see sampled instants: no flag
 * does not prove that nothing happened between two observes.
 *
 * Ordering is raft_engine_drain_committed's: every call runs on the engine
 * stream, sees every step enqueued before it, later step launches wait for
 * it, and it returns when its kernels have finished. */
#define RAFT_AUDIT_TERM_REGRESSED    (1 << 0)  /* a replica's currentTerm went backwards */
#define RAFT_AUDIT_VOTE_CHANGED      (1 << 1)  /* a replica changed its vote within a term */
#define RAFT_AUDIT_TWO_LEADERS       (1 << 2)  /* two leaders of one term, at once or across observes */
#define RAFT_AUDIT_COMMIT_CHANGED    (1 << 3)  /* a committed entry changed */
#define RAFT_AUDIT_LEADER_INCOMPLETE (1 << 4)  /* a newer leader lacks a committed entry */
typedef struct raft_audit raft_audit;
typedef struct raft_audit_info {         /* 64 bytes */
    int64_t newly_flagged;     /* groups whose flags went from 0 to nonzero in this call */
    int64_t flagged;           /* groups of the range with flags != 0 after it */
    int64_t term_regressed;    /* groups that gained the bit in this call, per kind */
    int64_t vote_changed;
    int64_t two_leaders;
    int64_t commit_changed;
    int64_t leader_incomplete;
    int64_t unknown;           /* checks skipped below a log_window */
} raft_audit_info;
typedef struct raft_audit_event {        /* 16 bytes */
    int64_t group;             /* engine-local group index */
    int32_t flags;
    int32_t first_step;
} raft_audit_event;
typedef struct raft_audit_report_info {  /* 64 bytes */
    int64_t delivered;         /* events written to out */
    int64_t pending;           /* flagged groups beyond max_events (all of them, in a peek) */
    int64_t flagged;           /* delivered + pending */
    int64_t reserved[5];       /* 0 */
} raft_audit_report_info;
int raft_audit_create (raft_engine* e, raft_audit** out);
int raft_audit_destroy(raft_audit* a);
int raft_audit_reset  (raft_audit* a);
int64_t raft_audit_device_bytes(raft_audit* a);
int raft_audit_observe(raft_audit* a, int64_t g0, int64_t n, raft_audit_info* info);
int raft_audit_report    (raft_audit* a, int64_t g0, int64_t n, raft_audit_event* out_host, int64_t max_events,
                          raft_audit_report_info* info);
int raft_audit_report_dev(raft_audit* a, int64_t g0, int64_t n, raft_audit_event* out_dev, int64_t max_events,
                          raft_audit_report_info* info);
int raft_audit_read (raft_audit* a, int64_t g0, int64_t n, int32_t* out);
int raft_audit_write(raft_audit* a, int64_t g0, int64_t n, const int32_t* in);

/* ---- the liveness monitor: outages, stalled commits and lag over time ---------
 * Additive to ABI 2 (RAFT_ABI_VERSION stays 2: nothing that existed changed).
 *
 * The audit above answers "did a group ever do something forbidden".  The
 * monitor answers the other half: which groups make no progress now, for how
 * long, and why -- so that raft_engine_append_noops, raft_engine_install_snapshot
 * and the transfers can be aimed at the groups that need them.
 * RAFT_C_GROUPS_WITH_LEADER is one number per step for the whole engine; the
 * monitor keeps, per group, since when it is down, and for the engine a
 * histogram of the lengths of the outages that ended.  The reference has no
 * counterpart.
 *
 * - A raft_monitor belongs to one engine and owns its HBM
 *   (raft_monitor_device_bytes: 64 G bytes of ledger rounded up to 256, and 512
 *   for the availability totals; raft_engine_device_bytes does not count it).
 *   The engine does not know about it: the step kernel, the canonical state,
 *   the digest and every other call are as before, raft_engine_reset does NOT
 *   reach it (call raft_monitor_reset), and it is destroyed before its engine.
 *   observe and report never write engine memory.
 * - The thresholds are fixed at create (raft_monitor_config).  RAFT_EINVAL: a
 *   null argument, a negative threshold, nonzero reserved, churn_terms > 0 with
 *   churn_steps < 1.
 * - The ledger of one group, 16 int32 words (64 bytes, whatever R) as
 *   raft_monitor_read returns it:
 *     [0]  now          RAFT_MONITOR_* bits true at the last observe          0
 *     [1]  ever         the sticky OR of every now                            0
 *     [2]  first_step   step index (low 32 bits) of the observe where ever
 *                       left 0                                                0
 *     [3]  leader       the newest leader at the last observe                 -1
 *     [4]  down_since   step index of the observe that first saw the running
 *                       outage                                                -1
 *     [5]  outages      outages that have ended (saturating)                  0
 *     [6]  down_total   the sum of their lengths in steps (saturating)        0
 *     [7]  longest      the longest of them                                   0
 *     [8]  stall_since  step index at which the running backlog last advanced -1
 *     [9]  stall_mark   the leader's committed prefix at that moment          0
 *     [10] win_start    the churn window's first step                         -1
 *     [11] win_term     the group's highest term at win_start                 0
 *     [12] lag_mask     bit r: replica r is lagging                           0
 *     [13] max_lag      the largest lag among the group's replicas            0
 *     [14], [15]        reserved                                              0
 *   (last column: the zero state of create and reset).
 * - One observe of one group, in this order; "old" is the ledger before the
 *   call.  s is the low 32 bits of raft_engine_step_index;
 *   age(x) = max(0, (int32)(s - x)) with the subtraction taken mod 2^32 (a step
 *   index that went backwards gives 0); L is the newest leader by
 *   raft_read_begin_batch's rule (role LEADER, the highest currentTerm, the
 *   lowest index among equals; -1 if none);
 *   hi_r = min(commitIndex_r, lastIndex_r) within 0..log_cap;
 *   T = max_r currentTerm_r.
 *   1. Outage.  L == -1: down_since = s if it was -1; LEADERLESS iff
 *      age(down_since) >= leaderless_steps.  L >= 0 and old down_since != -1: an
 *      outage ended, len = max(1, age(old down_since)); outages += 1,
 *      down_total += len, longest = max(longest, len), down_since = -1, and the
 *      monitor's availability totals get hist[floor(log2(len))] += 1,
 *      outages += 1, down_steps += len.  A fresh engine's wait for its first
 *      leader is an outage like any other.
 *   2. Stalled commit.  backlog = L >= 0 and lastIndex_L > hi_L.  No backlog:
 *      stall_since = -1, stall_mark = 0.  Backlog, and old stall_since == -1 or
 *      hi_L > old stall_mark: stall_since = s, stall_mark = hi_L.  Otherwise
 *      both stay: a new leader whose commit point is below the mark has not
 *      advanced anything.  COMMIT_STALLED iff backlog and
 *      age(stall_since) >= stalled_steps.  (What raft_engine_append_noops
 *      frees: a textbook leader whose log ends with an entry of an earlier
 *      term never commits it while idle.)
 *   3. Lag.  With lag_entries > 0 and L >= 0: lag_r = lastIndex_L - lastIndex_r
 *      for r != L; lag_mask has bit r iff lag_r >= lag_entries;
 *      max_lag = max(0, max_r lag_r) (at most 2^31 - 1); LAGGING iff
 *      lag_mask != 0.  Otherwise both words are 0.  (What
 *      raft_engine_install_snapshot(..., min_lag) heals.)
 *   4. Churn, only with churn_terms > 0.  If win_start == -1:
 *      (win_start, win_term) = (s, T).  CHURNING iff T - win_term >= churn_terms.
 *      Then, if age(win_start) >= churn_steps: (win_start, win_term) = (s, T).
 *   5. now = the bits above, ever |= now, first_step = s when ever leaves 0,
 *      leader = L.
 *   -1 means "none" in down_since, stall_since and win_start: an observe at a
 *   step index whose low 32 bits are 0xFFFFFFFF stores what reads as none.
 *   The rules read three state quads per replica (term and role, lastIndex,
 *   commitIndex) and no log slot: a log_window changes nothing and there is no
 *   `unknown` count.
 * - raft_monitor_report lists the groups of the range with (word & kinds) != 0
 *   -- word is now (RAFT_MONITOR_NOW) or ever (RAFT_MONITOR_EVER) -- in
 *   ascending group order, cut at max_events; `pending` counts the rest.  It
 *   consumes nothing; max_events == 0 (with or without a buffer) is a peek.
 *   RAFT_EINVAL also for another `which` and for bits in kinds outside
 *   RAFT_MONITOR_ALL.
 * - raft_monitor_get_availability / _set_availability read and resume the
 *   totals (hist[k]: ended outages of 2^k .. 2^(k+1) - 1 steps); a negative word
 *   or nonzero reserved: RAFT_EINVAL, nothing stored.
 * - raft_monitor_write resumes ledgers.  RAFT_EINVAL with nothing stored:
 *   unknown bits in now or ever, leader outside -1..R-1, lag_mask bits at or
 *   above R, negative outages, down_total, longest, max_lag or stall_mark,
 *   nonzero reserved words.  No ledger word is ever used as an index.
 * RAFT_EINVAL: null handle or info, max_events < 0, out == NULL with
 * max_events > 0, a _dev buffer that is not 16-byte aligned; RAFT_ERANGE:
 * groups outside the engine.  n == 0 is RAFT_OK with a zeroed info.
 *
 * Both protocol modes and every log layout.  The rules see sampled instants:
 * an outage's length is measured between the observe that first saw no leader
 * and the observe that first saw one again, a leader lost and regained between
 * two observes is never seen, and observing every k steps measures in units of
 * k.  Observed after every step with leaderless_steps = 0, info.leaderless is
 * G - RAFT_C_GROUPS_WITH_LEADER of that step.
 *
 * Ordering is raft_engine_drain_committed's: every call runs on the engine
 * stream, sees every step enqueued before it, later step launches wait for
 * it, and it returns when its kernels have finished. */
#define RAFT_MONITOR_LEADERLESS     (1 << 0)  /* no LEADER for leaderless_steps steps or more */
#define RAFT_MONITOR_COMMIT_STALLED (1 << 1)  /* the leader's backlog has not advanced for stalled_steps steps */
#define RAFT_MONITOR_LAGGING        (1 << 2)  /* a replica is lag_entries or more behind the newest leader */
#define RAFT_MONITOR_CHURNING       (1 << 3)  /* the highest term rose by churn_terms within a window */
#define RAFT_MONITOR_ALL            15
#define RAFT_MONITOR_NOW  0
#define RAFT_MONITOR_EVER 1
typedef struct raft_monitor raft_monitor;
typedef struct raft_monitor_config {     /* 32 bytes */
    int32_t leaderless_steps;  /* LEADERLESS once a group has shown no LEADER for this many steps (0: at once) */
    int32_t stalled_steps;     /* COMMIT_STALLED once a backlog has not advanced for this many steps */
    int32_t lag_entries;       /* LAGGING: a replica this many entries behind the newest leader (0: off) */
    int32_t churn_terms;       /* CHURNING: the group's highest term rose by this much within a window (0: off) */
    int32_t churn_steps;       /* the window's length in steps (>= 1 when churn_terms > 0) */
    int32_t reserved[3];       /* 0 */
} raft_monitor_config;
typedef struct raft_monitor_info {       /* 96 bytes */
    int64_t flagged;           /* groups of the range with now != 0 after the call */
    int64_t newly_flagged;     /* old now == 0, now != 0 */
    int64_t cleared;           /* old now != 0, now == 0 */
    int64_t leaderless;        /* groups with the bit in now, per kind */
    int64_t commit_stalled;
    int64_t lagging;
    int64_t churning;
    int64_t down;              /* groups with down_since != -1 after the call (flagged or not yet) */
    int64_t outages_ended;     /* by this call */
    int64_t down_steps_ended;  /* the sum of their lengths */
    int64_t reserved[2];       /* 0 */
} raft_monitor_info;
typedef struct raft_monitor_event {      /* 32 bytes */
    int64_t group;             /* engine-local group index */
    int32_t now, ever, down_since, stall_since, leader, lag_mask;
} raft_monitor_event;
typedef struct raft_monitor_report_info {  /* 64 bytes */
    int64_t delivered;         /* events written to out */
    int64_t pending;           /* listed groups beyond max_events (all of them, in a peek) */
    int64_t flagged;           /* delivered + pending */
    int64_t reserved[5];       /* 0 */
} raft_monitor_report_info;
typedef struct raft_monitor_availability {  /* 288 bytes */
    int64_t hist[32];          /* hist[k]: ended outages whose length in steps has floor(log2) == k */
    int64_t outages;           /* ended outages */
    int64_t down_steps;        /* the sum of their lengths */
    int64_t reserved[2];       /* 0 */
} raft_monitor_availability;
int raft_monitor_create (raft_engine* e, const raft_monitor_config* cfg, raft_monitor** out);
int raft_monitor_destroy(raft_monitor* m);
int raft_monitor_reset  (raft_monitor* m);
int64_t raft_monitor_device_bytes(raft_monitor* m);
int raft_monitor_observe(raft_monitor* m, int64_t g0, int64_t n, raft_monitor_info* info);
int raft_monitor_report    (raft_monitor* m, int64_t g0, int64_t n, int32_t which, int32_t kinds,
                            raft_monitor_event* out_host, int64_t max_events, raft_monitor_report_info* info);
int raft_monitor_report_dev(raft_monitor* m, int64_t g0, int64_t n, int32_t which, int32_t kinds,
                            raft_monitor_event* out_dev, int64_t max_events, raft_monitor_report_info* info);
int raft_monitor_get_availability(raft_monitor* m, raft_monitor_availability* out);
int raft_monitor_set_availability(raft_monitor* m, const raft_monitor_availability* in);
int raft_monitor_read (raft_monitor* m, int64_t g0, int64_t n, int32_t* out);
int raft_monitor_write(raft_monitor* m, int64_t g0, int64_t n, const int32_t* in);

/* ---- the persistence stream: hard state and new log entries as a delta ----------
 * Additive to ABI 2 (RAFT_ABI_VERSION stays 2: nothing that existed changed).
 *
 * What a replica must make durable before its answers count: currentTerm,
 * votedFor and the log entries it gained or replaced since the last poll --
 * etcd's Ready.HardState and Ready.Entries, beside Ready.CommittedEntries
 * (raft_engine_drain_committed) and SoftState (raft_engine_poll_leaders).  It
 * is what raft_engine_restart's "term, vote and log persist" stands on: a host
 * that applies the stream to an image can write a replica back after
 * RAFT_RESTART_AMNESIA, keep a write-ahead log, or keep a second engine in
 * step, without copying every log row.  The reference persists nothing.
 *
 * - A raft_wal belongs to one engine and owns its HBM (raft_wal_device_bytes:
 *   24 G R bytes of cursors rounded up to 256; raft_engine_device_bytes does not
 *   count it).  The engine does not know about it: the step kernel, the
 *   canonical state, the digest and every other call are as before,
 *   raft_engine_reset does NOT reach it (call raft_wal_reset), and it is
 *   destroyed before its engine.  A poll never writes engine memory.
 * - The cursor of one replica (raft_wal_cursor, 24 bytes; fresh: 0, -1, 0, 0, 0):
 *     term, vote    the hard state last handed out
 *     stable        a count, like commitIndex: entries [0, stable) have been
 *                   handed out as they were at the time
 *     stable_term   the term of entry stable - 1 as handed out (0 at stable 0)
 *     floor         a count <= stable: entries [0, floor) were committed on
 *                   this replica when handed out
 * - A poll visits the selected replicas of groups [g0, g0 + n) (replica = -1:
 *   every replica, else that index of each group).  For each, with the state
 *   now, last = clamp(lastIndex, 0, log_cap), hi the committed prefix of
 *   raft_engine_drain_committed and, with a log_window W,
 *   wl = max(0, physLen - W) (else 0):
 *   the replica is CLEAN when stable <= last and either stable == 0 or slot
 *   stable - 1 is readable (>= wl) and log[stable - 1].term == stable_term.
 *   1. If (currentTerm, votedFor) != (term, vote): one RAFT_WAL_HARDSTATE.
 *   2. If not clean: keep = min(floor, last); keep < floor means committed
 *      entries vanished (amnesia, reference-mode quirks) and counts the replica
 *      in `regressed`; one RAFT_WAL_TRUNCATE(keep); from here on stable = keep.
 *   3. Entries stable .. last - 1 follow, ascending, one RAFT_WAL_ENTRY each.
 *      On a ring the ones below wl cannot be read: they are counted in `lost`,
 *      not emitted, and the call returns RAFT_EWINDOW after doing everything
 *      else (as the drain does).
 *   Why floor is enough without a shadow copy of the log: by Log Matching two
 *   logs that agree on the term at one index agree on everything before it,
 *   so the one comparison at stable - 1 proves that the whole handed-out
 *   prefix is still the replica's log.  A replica's own committed prefix is
 *   final in RAFT_MODE_TEXTBOOK, so after any mismatch re-sending from floor is
 *   always sufficient; it is more than necessary only by the part of the
 *   uncommitted suffix that did not change.
 * - Records come in ascending (group, replica) order and, inside a replica, as
 *   HARDSTATE, TRUNCATE, ENTRY ascending.  When there are more than
 *   max_records, exactly the first max_records are written (the cut may fall
 *   anywhere, also between a replica's HARDSTATE and its TRUNCATE) and
 *   `pending` counts the rest.  The cursor advances only past what was written:
 *   a written HARDSTATE stores term / vote; a written TRUNCATE stores
 *   stable = keep and stable_term = log[keep - 1].term (0 at keep == 0 or below
 *   wl); each written ENTRY moves stable and stable_term.  After the call every
 *   visited replica whose handed-out prefix is its log -- it was clean, or its
 *   TRUNCATE was written -- gets floor = min(hi, stable); one whose TRUNCATE
 *   was cut off keeps its cursor's stable and floor.  With no step in between,
 *   successive polls concatenated equal one poll with enough room, record for
 *   record and cursor for cursor (on a ring that lost entries a TRUNCATE whose
 *   entries were cut off is sent again, and `lost` counts them again).
 *   out == NULL with max_records == 0 is a peek: nothing is stored, `pending`
 *   / `lost` / `regressed` say what a poll would see.
 * - Promised: in RAFT_MODE_TEXTBOOK without RAFT_RESTART_AMNESIA, applying the
 *   records of successive polls to an empty image (TRUNCATE(keep): drop every
 *   entry at index >= keep; ENTRY: store at its index) yields exactly the
 *   replica's currentTerm, votedFor and log [0, lastIndex) as of the last
 *   poll; on a ring, the retained window of it.  Not promised: in
 *   RAFT_MODE_REFERENCE (quirks Q1-Q4, Q9 rewrite committed entries and terms
 *   repeat across leaders) and after an amnesia restart the stream is defined
 *   and deterministic, and `regressed` says where committed entries vanished,
 *   but the image may differ from the log below floor.
 * - raft_wal_read / raft_wal_write export and resume cursors ([n][R], as they
 *   lie on the device).  raft_wal_write refuses, with RAFT_EINVAL and nothing
 *   stored: stable outside 0..log_cap, floor outside 0..stable, vote outside
 *   -1..R (votedFor holds a node id, replica index + 1, RaftServer.kt:193: the
 *   step kernel stores -1 or 1..R), term < 0, a nonzero pad.  raft_wal_reset:
 *   every cursor fresh.
 * RAFT_EINVAL: null handle or info, replica outside -1..R-1, max_records < 0,
 * out == NULL with max_records > 0, a _dev buffer that is not 8-byte aligned;
 * RAFT_ERANGE: groups outside the engine.  n == 0 is RAFT_OK with a zeroed info.
 *
 * Ordering is raft_engine_drain_committed's: every call runs on the engine
 * stream, sees every step enqueued before it, later step launches wait for
 * it, and it returns when its kernels have finished (info stays a host
 * pointer in the _dev variant). */
#define RAFT_WAL_HARDSTATE 0   /* term = currentTerm, aux = votedFor, index = -1, cmd = 0: persist this pair */
#define RAFT_WAL_TRUNCATE  1   /* index = keep, the rest 0: drop every persisted entry at index >= keep */
#define RAFT_WAL_ENTRY     2   /* index, term, cmd as the log holds them, aux = 0: persist this entry */
typedef struct raft_wal raft_wal;
typedef struct raft_wal_cursor {   /* 24 bytes */
    int32_t term, vote, stable, stable_term, floor, pad;
} raft_wal_cursor;
typedef struct raft_wal_record {   /* 24 bytes */
    int32_t  group;                /* engine-local group index */
    int16_t  replica;
    int16_t  kind;                 /* RAFT_WAL_* */
    int32_t  index;
    int32_t  term;
    uint32_t cmd;
    int32_t  aux;
} raft_wal_record;
typedef struct raft_wal_info {     /* 56 bytes */
    int64_t delivered;             /* records written to out */
    int64_t pending;               /* records left for lack of room (all of them, in a peek) */
    int64_t hardstates;            /* of the records written, per kind */
    int64_t truncates;
    int64_t entries;
    int64_t lost;                  /* log_window only: entries that left the window unpersisted; skipped */
    int64_t regressed;             /* selected replicas whose TRUNCATE goes below their floor */
} raft_wal_info;
int raft_wal_create (raft_engine* e, raft_wal** out);
int raft_wal_destroy(raft_wal* w);
int raft_wal_reset  (raft_wal* w);
int64_t raft_wal_device_bytes(raft_wal* w);
int raft_wal_poll    (raft_wal* w, int64_t g0, int64_t n, int32_t replica, raft_wal_record* out_host,
                      int64_t max_records, raft_wal_info* info);
int raft_wal_poll_dev(raft_wal* w, int64_t g0, int64_t n, int32_t replica, raft_wal_record* out_dev,
                      int64_t max_records, raft_wal_info* info);
int raft_wal_read (raft_wal* w, int64_t g0, int64_t n, raft_wal_cursor* cursors);
int raft_wal_write(raft_wal* w, int64_t g0, int64_t n, const raft_wal_cursor* cursors);

/* ---- scripted network faults: isolate chosen replicas, heal, list ---------------
 * Additive to ABI 2 (RAFT_ABI_VERSION stays 2: nothing that existed changed).
 *
 * The network faults of raft_engine_create are rates (drop_ppm, churn_ppm,
 * partition_period).  These calls aim the one fault the engine keeps a word
 * for: a group's isolation word, rem << 8 | replica (word 0 of the group's
 * RAFT_GROUP_EXTRA in the canonical state), which cuts every message to and
 * from that replica while it runs.  It is the word the churn harness sets for
 * the lowest LEADER, raft_engine_restart sets for down_steps and
 * raft_transfer_batch reads (RAFT_TRANSFER_UNREACHABLE); the step kernel, the
 * digest and the canonical state are as before, and an engine that never calls
 * these behaves as before, byte for byte.  The isolated replica keeps its state
 * and its timers run: a cut-off leader goes on calling itself LEADER (what
 * raft_engine_sm_get then answers from, and raft_read_begin_batch does not).
 *
 * - A word is RUNNING when rem > 0.  At the start of every step a running word
 *   counts down by one and, while rem is still above 0, cuts the replica for
 *   that step; at rem == 0 the whole word becomes 0.  So a word set to `steps`
 *   between two steps cuts the next steps - 1 steps and is gone after `steps`
 *   (raft_engine_restart's down_steps counts the same way).
 * - There is one word per group: at most one replica of a group is isolated at
 *   a time, by whoever wrote last (these calls, down_steps, the churn harness,
 *   raft_engine_write_state).  With churn_ppm > 0 the harness isolates only in
 *   groups whose word has run out.  Two-way partitions cannot be scripted: the
 *   step kernel draws them from Philox per window (RAFT_RNG_PARTITION) and keeps
 *   no word for them.
 *
 * raft_isolate_batch: one message per entry, "isolate target[m] of group[m]
 * for steps[m]".  target 0..R-1 names a replica; RAFT_ISOLATE_NEWEST_LEADER is
 * the LEADER of the highest currentTerm, the lowest index among equals
 * (raft_read_begin_batch's and the watch's rule); RAFT_ISOLATE_LOWEST_LEADER is
 * raft_leader_info.leader, the replica the churn harness would hit.  steps is in
 * 1..RAFT_ISOLATE_MAX_STEPS.  Every message is judged against the state before
 * the call, and per group only ONE message is judged: the one at the lowest
 * batch position among the group's messages that are in range.  The ticket:
 *   INVALID     target or steps out of range; nothing of the group is read and
 *               the message takes no part in the choice above.  (-1, steps, 0)
 *   DUPLICATE   an earlier message of the batch to the same group was judged;
 *               prev is ITS BATCH POSITION.  (-1, steps, position)
 *   NO_LEADER   a leader selector found no LEADER.  (-1, steps, word found)
 *   BUSY        the word found is running and flags lacks RAFT_ISOLATE_REPLACE;
 *               nothing is written.  (replica resolved, steps, word found)
 *   SET         the word is now steps << 8 | replica.  (replica, steps, word found)
 * in that order of precedence.  A group outside the engine fails the call with
 * RAFT_ERANGE before a word or a ticket is written, as in the handler batches.
 * RAFT_EINVAL: null engine, a null array with n > 0, n < 0 or >= 2^31, flag
 * bits other than RAFT_ISOLATE_REPLACE, a _dev ticket buffer that is not
 * 16-byte aligned.  n == 0 is RAFT_OK.
 *
 * raft_engine_heal_network: for every group of [g0, g0 + n) whose word is
 * running and whose isolated replica r has bit r set in mask[j] (NULL: any
 * replica), the word becomes 0 -- exactly what the step kernel's own expiry
 * leaves -- and the replica hears and is heard from the next step on.  info
 * counts the groups healed, idle (no running word; nothing is written, a stale
 * replica byte included) and kept (running, not selected).
 *
 * raft_engine_list_isolated: the groups of [g0, g0 + n) with a running word as
 * raft_isolated records in ascending group order, at most max_events of them;
 * `running` counts them all and `pending` those left out.  out == NULL with
 * max_events == 0 is a peek.  Read-only.  role is the isolated replica's role
 * now (-1 if a written word names a replica outside the group).
 *
 * RAFT_EINVAL for heal and list: null engine or info, max_events < 0, out ==
 * NULL with max_events > 0, a _dev record buffer that is not 16-byte aligned;
 * RAFT_ERANGE: groups outside the engine.  n == 0 is RAFT_OK with a zeroed info.
 *
 * Ordering is raft_engine_drain_committed's: every call runs on the engine
 * stream, sees every step enqueued before it, later step launches wait for it,
 * and it returns when its kernels have finished.  The _dev forms take DEVICE
 * pointers under the buffer rules of raft_*_batch_dev (info stays a host
 * pointer). */
#define RAFT_ISOLATE_NEWEST_LEADER (-1)  /* target: the LEADER of the highest currentTerm */
#define RAFT_ISOLATE_LOWEST_LEADER (-2)  /* target: the lowest replica index whose role is LEADER */
#define RAFT_ISOLATE_REPLACE        1    /* flags: overwrite a running isolation instead of answering BUSY */
#define RAFT_ISOLATE_MAX_STEPS      0x7FFFFF  /* 2^23 - 1, raft_engine_restart's largest down_steps */
#define RAFT_ISOLATE_SET            0
#define RAFT_ISOLATE_BUSY           1
#define RAFT_ISOLATE_NO_LEADER      2
#define RAFT_ISOLATE_DUPLICATE      3
#define RAFT_ISOLATE_INVALID        4
typedef struct raft_isolate_ticket {   /* 16 bytes */
    int32_t replica;  /* the replica named or resolved (-1: none) */
    int32_t steps;    /* as given */
    int32_t status;   /* RAFT_ISOLATE_SET ... RAFT_ISOLATE_INVALID */
    int32_t prev;     /* the isolation word found; DUPLICATE: the judged message's batch position; INVALID: 0 */
} raft_isolate_ticket;
int raft_isolate_batch    (raft_engine* e, const int64_t* group, const int32_t* target, const int32_t* steps,
                           int32_t flags, raft_isolate_ticket* ticket, int64_t n);
int raft_isolate_batch_dev(raft_engine* e, const int64_t* group, const int32_t* target, const int32_t* steps,
                           int32_t flags, raft_isolate_ticket* ticket, int64_t n);
typedef struct raft_heal_info {        /* 32 bytes */
    int64_t healed;       /* groups whose running word was cleared */
    int64_t idle;         /* groups with no running word */
    int64_t kept;         /* groups whose running word names a replica outside the mask */
    int64_t reserved;     /* 0 */
} raft_heal_info;
int raft_engine_heal_network    (raft_engine* e, int64_t g0, int64_t n, const uint8_t* mask_host, raft_heal_info* info);
int raft_engine_heal_network_dev(raft_engine* e, int64_t g0, int64_t n, const uint8_t* mask_dev, raft_heal_info* info);
typedef struct raft_isolated {         /* 16 bytes */
    int64_t group;        /* engine-local group index */
    int16_t replica;      /* the isolated replica */
    int16_t role;         /* its role now (RAFT_FOLLOWER / RAFT_CANDIDATE / RAFT_LEADER) */
    int32_t remaining;    /* rem of the word: it cuts the next remaining - 1 steps */
} raft_isolated;
typedef struct raft_isolated_info {    /* 32 bytes */
    int64_t delivered;    /* records written to out */
    int64_t pending;      /* running - delivered */
    int64_t running;      /* groups of the range with a running word */
    int64_t reserved;     /* 0 */
} raft_isolated_info;
int raft_engine_list_isolated    (raft_engine* e, int64_t g0, int64_t n, raft_isolated* out_host, int64_t max_events,
                                  raft_isolated_info* info);
int raft_engine_list_isolated_dev(raft_engine* e, int64_t g0, int64_t n, raft_isolated* out_dev, int64_t max_events,
                                  raft_isolated_info* info);

/* ---- single-handler batches: the service boundary ----------------------
 * group: engine-local group index; dst: replica index 0..R-1.  Messages
 * to the same (group, dst) are applied in batch order.  Effects on the
 * consumer (timer reset) use the engine's current step index.  With a
 * log_window, a batch in which some handler touched a slot below its
 * replica's window returns RAFT_EWINDOW after applying it. */
int raft_vote_batch(raft_engine* e, const int64_t* group, const int32_t* dst,
                    const raft_vote_req* req, raft_vote_resp* resp, int64_t n);
int raft_append_batch(raft_engine* e, const int64_t* group, const int32_t* dst,
                      const raft_append_req* req, raft_append_resp* resp, int64_t n);
/* appendCommand (RaftServer.kt:100-107): log.add(lastIndex, (currentTerm, cmd)). */
int raft_append_command_batch(raft_engine* e, const int64_t* group, const int32_t* replica,
                              const uint32_t* cmd, int64_t n);
/* Page-locked host memory for batch arrays: the host entry points above move
 * arrays that live in it by direct DMA (no staging copy; ≈3-5x the rate of
 * pageable arrays at 10^6 messages).  A JNI adapter wraps it in a direct
 * ByteBuffer.  raft_host_alloc returns NULL on failure
 * (raft_last_error() says why). */
void* raft_host_alloc(int64_t bytes);
int   raft_host_free(void* p);
/* The same three on DEVICE buffers of this engine's GPU (group, dst/replica,
 * req, resp: n entries each, in HBM), enqueued on the engine stream; they
 * return once the batch finished.  The engine stream is non-blocking: it does
 * NOT wait for work on other streams, so the device buffers must be complete
 * (and resp no longer in use) before the call -- produced on the engine
 * stream, synchronised, or ordered with raft_engine_wait_stream().  The host
 * entry points above stage their buffers through engine-owned pinned memory
 * and call these.  A message whose group or replica is outside the engine
 * makes the whole batch fail with RAFT_ERANGE before any message is applied.
 * n < 2^31. */
/* Order the engine stream after all work enqueued so far on `stream` (a
 * hipStream_t as void*, NULL = the null stream): later engine calls see that
 * work's results.  Host-side and non-blocking (an event record and wait). */
int raft_engine_wait_stream(raft_engine* e, void* stream);
int raft_vote_batch_dev(raft_engine* e, const int64_t* group, const int32_t* dst,
                        const raft_vote_req* req, raft_vote_resp* resp, int64_t n);
int raft_append_batch_dev(raft_engine* e, const int64_t* group, const int32_t* dst,
                          const raft_append_req* req, raft_append_resp* resp, int64_t n);
int raft_append_command_batch_dev(raft_engine* e, const int64_t* group, const int32_t* replica,
                                  const uint32_t* cmd, int64_t n);
/* How the batches above order messages (results never depend on it):
 * RAFT_BATCH_PATH_SORTED, a stable radix sort of every message by
 * (group, replica); RAFT_BATCH_PATH_BUCKETED, one stable partition into
 * buckets of 2^S consecutive replicas, each bucket sorted in LDS by the
 * workgroup that applies it (G * R <= 2^32 only, else RAFT_EINVAL at the
 * batch); RAFT_BATCH_PATH_AUTO (the default): bucketed where it applies. */
#define RAFT_BATCH_PATH_AUTO     0
#define RAFT_BATCH_PATH_SORTED   1
#define RAFT_BATCH_PATH_BUCKETED 2
int raft_engine_set_batch_path(raft_engine* e, int32_t path);

/* ---- Philox4x32-10 (shared bit-for-bit with the CPU harness) -----------
 * Counter = (c0 = step, c1 = global group id, c2 = purpose, c3 = sub),
 * key = (seed lo32, seed hi32).  Purposes: */
#define RAFT_RNG_TIMER        1u  /* sub = replica >> 2, word replica & 3: the replica's
                                     per-step draw, scaled to the election timeout or to
                                     the backoff (never both in one step)               */
#define RAFT_RNG_BACKOFF      2u  /* reserved (the backoff shares the timer word)      */
#define RAFT_RNG_VOTE_DROP    3u  /* sub = src | chunk << 8: 16-bit drop uniforms */
#define RAFT_RNG_APPEND_DROP  4u  /* sub = src | chunk << 8                        */
#define RAFT_RNG_HARNESS      5u  /* sub = 0: w0 churn, w1 command, w2 command id  */
#define RAFT_RNG_PARTITION    6u  /* c0 = partition window start, sub = 0: w0 mask */
#define RAFT_RNG_RESTART      7u  /* c0 = step index at the call, sub = replica >> 2, word
                                     replica & 3: raft_engine_restart_random's selection */
#define RAFT_RNG_INIT_STEP    0xFFFFFFFFu  /* c0 of the initial timer draws        */
void raft_philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]);

#ifdef __cplusplus
}
#endif
#endif /* RAFT_ENGINE_H */
