/* raft_debug.h — extension of the engine's C-ABI (include/raft_engine.h): a
 * read-only window on words of the engine that no accessor exports.  The entry
 * point lives in the same library (libraft_engine.so); this header only adds a
 * declaration. */
#ifndef RAFT_EXT_DEBUG_H
#define RAFT_EXT_DEBUG_H

#include "../raft_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the log-tail cache, as it lies in HBM ---------------------------------------
 * Additive to ABI 2 (RAFT_ABI_VERSION stays 2: nothing that existed changed).
 * An extension header: it includes raft_engine.h and adds a declaration only; a
 * host that never includes it sees the C-ABI it always saw.
 *
 * Every replica carries three words beside its canonical fields: t1 and t2, the
 * terms of log[lastIndex - 1] and log[lastIndex - 2], and c1, the command of
 * log[lastIndex - 1].  The step kernel, the handler batches, the routed
 * proposals, leadership transfer and the no-op entries read them instead of the
 * log; every device-side writer of lastIndex or of the log keeps them.  A host
 * write (raft_engine_write_state / raft_engine_write_log) marks them stale and
 * the next consumer rebuilds them from the log first.  raft_engine_read_state
 * does not export them (the canonical layout stays), so a test that wants to
 * hold a writer to "cache == what the log says" reads them here.
 *
 * raft_debug_read_tail_cache copies the three words of every replica of groups
 * [g0, g0 + n) into out[n][R][3] (t1, t2, c1; c1's bits as int32_t), on the
 * engine stream: after every step and side-path call enqueued before it.
 * *valid = 1 when the engine holds the cache to be current, 0 when a host write
 * left it stale and no consumer has run since (the words are then whatever the
 * last writer left).  The call rebuilds nothing and writes no word of engine
 * state or of that flag: two calls in a row return the same.  A test window: it
 * is not timed and promises no speed.
 * RAFT_EINVAL: null engine, null out with n > 0, null valid.  RAFT_ERANGE: a
 * group range outside the engine.  n == 0 stores *valid and is RAFT_OK. */
int raft_debug_read_tail_cache(raft_engine* e, int64_t g0, int64_t n, int32_t* out, int32_t* valid);

#ifdef __cplusplus
}
#endif

#endif  /* RAFT_EXT_DEBUG_H */
