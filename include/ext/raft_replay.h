/* raft_replay.h — extension of the engine's C-ABI (include/raft_engine.h): WAL
 * replay, the inverse of the persistence stream's poll.  The entry points live
 * in the same library (libraft_engine.so); this header only adds declarations. */
#ifndef RAFT_EXT_REPLAY_H
#define RAFT_EXT_REPLAY_H

#include "../raft_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- WAL replay: rebuild replicas on the device from the stream -----------------
 * Additive to ABI 2 (RAFT_ABI_VERSION stays 2: nothing that existed changed).
 * An extension header: it includes raft_engine.h and adds declarations only; a
 * host that never includes it sees the C-ABI it always saw.
 *
 * The inverse of raft_wal_poll: one call applies a batch of raft_wal_records
 * to the replicas they name, in HBM, between two step launches.  A replica
 * gets back what it had persisted after RAFT_RESTART_AMNESIA in one kernel
 * pair instead of a read_state / read_log / write_log / write_state of its
 * whole group (and without the engine-wide cache rebuild a write_state costs),
 * and raft_wal_poll_dev feeding raft_wal_replay_dev keeps a second engine in
 * step with no host copy of a record.  The call belongs to the TARGET engine
 * and needs no raft_wal handle; the records may come from another engine of
 * the same R, mode, log_cap and log_window.  The step kernel, the persistence
 * stream and the digest are as before.
 *
 * - The batch: n records in ascending (group, replica) order; inside one
 *   replica's run at most one HARDSTATE, then at most one TRUNCATE, then
 *   ENTRYs with index rising by exactly 1.  That is what one raft_wal_poll
 *   emits, and what the pieces max_records cuts out of a poll give,
 *   concatenated or sent one call after another.
 * - A record is MALFORMED when: it breaks that order; its group is outside
 *   the engine or its replica outside 0..R-1; its kind is unknown; it is a
 *   HARDSTATE with term < 0 or aux outside -1..R; a TRUNCATE whose keep
 *   (index) is outside 0..lastIndex of the target now; an ENTRY with index
 *   outside 0..log_cap-1; an ENTRY that follows neither a TRUNCATE nor an
 *   ENTRY of its run and whose index is not the target's lastIndex now (with
 *   a log_window: is below it -- above it is accepted, the entries between
 *   left the source's window unpersisted and raft_wal_poll counted them in
 *   `lost`); an ENTRY after a TRUNCATE whose index is not keep; with a
 *   log_window W, an ENTRY whose successor W records later lies in the same
 *   run (one poll never emits more than W entries of a replica; two records
 *   of a batch then never share a ring slot).  lastIndex is taken within
 *   0..log_cap.  Every check looks at a record, its neighbours and the
 *   target's state words.  ONE malformed record fails the whole batch with
 *   RAFT_EINVAL, info->malformed = how many there are and every other word of
 *   info 0, before anything is written (as an out-of-range group does in the
 *   handler batches).
 * - The effect on a replica the batch touches, in raft_engine_read_state /
 *   raft_engine_read_log words: currentTerm and votedFor come from its
 *   HARDSTATE if it has one, else they stay.  lastIndex and physLen are set
 *   from the last record of its run -- an ENTRY's index + 1, else the
 *   TRUNCATE's keep, else both stay.  Each ENTRY's (term, cmd) is stored at
 *   slot index.  The volatile state is what raft_engine_restart with flags 0
 *   leaves: FOLLOWER, commitIndex 0, RAFT_FL_ARMED alone, phaseMs = retryMs =
 *   0, a fresh electionMs from the replica's RAFT_RNG_TIMER word at the
 *   target's step index, rows next[r][*] and match[r][*] zero, the primary
 *   session slot given up if the replica owned it: a replica that reads its
 *   disk is a replica that starts.  lastApplied and the machine are not
 *   touched (they are durable consumers; their `regressed` rules cover a log
 *   that got shorter).  Replicas the batch does not name do not change.  The
 *   engine's internal mirrors (the log-tail cache, the session rows'
 *   placement) end up as raft_engine_write_state + raft_engine_write_log of
 *   the same words leave them, without their engine-wide rebuild.
 * - flags: RAFT_REPLAY_KEEP_VOLATILE applies the persistent words and the log
 *   and leaves role, commitIndex, flags, timers and sessions alone: for
 *   feeding a standby that is never stepped.  Unknown bits: RAFT_EINVAL.
 * - Promised: in RAFT_MODE_TEXTBOOK without RAFT_RESTART_AMNESIA on the
 *   source, replaying every record of every poll of engine A, in order, into
 *   a fresh engine B of the same parameters gives B the persistent state of A
 *   as of A's last poll -- currentTerm, votedFor, lastIndex and the log
 *   [0, lastIndex), on a ring the retained window of it.  So B equals A after
 *   every replica of A restarted with its disk intact -- with two
 *   qualifications.  electionMs is drawn at the step index of the replay that
 *   touches a replica: B's timeouts are those of A's restart only for the
 *   replicas a replay touched at that step index (a HARDSTATE of a replica's
 *   own term and vote touches it and changes nothing else).  And physLen
 *   becomes lastIndex: slots a flat log of A keeps past lastIndex are not in
 *   the stream.  In RAFT_MODE_REFERENCE
 *   the call is defined and deterministic and nothing more is promised, as
 *   for the poll.
 * RAFT_EINVAL: null engine or info, n < 0 or n >= 2^31, a null buffer with
 * n > 0, unknown flag bits, a _dev buffer that is not 8-byte aligned, a
 * malformed record.  n == 0 is RAFT_OK with a zeroed info.
 *
 * Ordering is raft_engine_restart's: the call runs on the engine stream, sees
 * every step enqueued before it, later step launches wait for it, and it
 * returns when its kernels have finished.  raft_wal_replay_dev takes a DEVICE
 * pointer under the buffer rules of raft_*_batch_dev (info stays a host
 * pointer). */
#define RAFT_REPLAY_KEEP_VOLATILE 1  /* flags: leave role, commitIndex, flags, timers and sessions as they are */
typedef struct raft_replay_info {  /* 64 bytes */
    int64_t applied;               /* records applied (n, or 0 when the batch was refused) */
    int64_t replicas;              /* distinct (group, replica) touched */
    int64_t hardstates;            /* of the records applied, per kind */
    int64_t truncates;
    int64_t entries;
    int64_t malformed;             /* records that broke a rule: > 0 only with RAFT_EINVAL, nothing written */
    int64_t reserved[2];           /* 0 */
} raft_replay_info;
int raft_wal_replay    (raft_engine* e, const raft_wal_record* rec_host, int64_t n, uint32_t flags,
                        raft_replay_info* info);
int raft_wal_replay_dev(raft_engine* e, const raft_wal_record* rec_dev, int64_t n, uint32_t flags,
                        raft_replay_info* info);

#ifdef __cplusplus
}
#endif

#endif  /* RAFT_EXT_REPLAY_H */
