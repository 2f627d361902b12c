// raft_debug.hip — a read-only window on the log-tail cache
// (include/ext/raft_debug.h raft_debug_read_tail_cache): the words t1, t2 and
// c1 of every replica of a group range, as they lie in HBM, and the engine's
// cache_valid flag.  One kernel, one thread per replica, three loads and three
// stores; the words come back through the host calls' staging (Staged).  It
// never calls raft_internal_ensure_cache and stores nothing into the state: the
// tests hold every device-side writer of the cache to rebuild_cache_kernel's
// rule with it (tests/tail_cache_model.py).
#include <hip/hip_runtime.h>

#include "ext/raft_debug.h"
#include "raft_engine_impl.h"

using namespace raft;

namespace {

// replicas [i0, i0 + n) of the engine (i0 + n <= GR: check_groups); out[j] = (t1, t2, c1) of replica i0 + j
__global__ __launch_bounds__(BLOCK) void read_tail_cache_kernel(DevParams p, int64_t i0, int64_t n,
                                                                int32_t* __restrict__ out) {
    const int64_t j = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n) return;
    const int64_t idx = i0 + j;
    out[3 * j] = p.st[fidx(p, F_T1, idx)];
    out[3 * j + 1] = p.st[fidx(p, F_T2, idx)];
    out[3 * j + 2] = p.st[fidx(p, F_C1, idx)];
}

}  // namespace

extern "C" int raft_debug_read_tail_cache(raft_engine* e, int64_t g0, int64_t n, int32_t* out, int32_t* valid) {
    if (int rc = check_groups(e, g0, n)) return rc;
    if (!valid) return raft_internal_fail(RAFT_EINVAL, "null valid");
    if (n > 0 && !out) return raft_internal_fail(RAFT_EINVAL, "null buffer");
    *valid = e->cache_valid ? 1 : 0;
    if (n == 0) return RAFT_OK;
    HIP_TRY(hipSetDevice(e->device));
    e->fork_needed = true;                           // later step launches wait for the read
    const int64_t reps = n * e->p.R;
    const Staged s{{0, 0, 0}, 0, (size_t)reps * 3 * sizeof(int32_t)};   // no input: the output at offset 0
    if (int rc = raft_internal_grow_dev(e, &e->cio, &e->cio_bytes, s.out_bytes)) return rc;
    if (int rc = raft_internal_grow_host(e, &e->hst, &e->hst_bytes, s.out_bytes)) return rc;
    read_tail_cache_kernel<<<(unsigned)((reps + BLOCK - 1) / BLOCK), BLOCK, 0, e->stream>>>(
        e->dp, g0 * e->p.R, reps, (int32_t*)(e->cio + s.out_off));
    HIP_TRY(hipGetLastError());
    return stage_out(e, s, out);
}
