// raft_ledger.h — internal to the engine library, not installed: what the side
// paths that keep a table per group (or per replica) beside the engine share.
//   raft_audit.hip, raft_monitor.hip, raft_wal.hip   a handle each (raft_ledger), its tables, observe / report
//   raft_apply.hip, raft_watch.hip, raft_sm.hip, raft_outbox.hip   the table copies of their read / write pairs
//   raft_nemesis.hip   the listing's shell
// A new ledger is a layout, a fill kernel and the rules of a row (DESIGN.md
// §4.26); the lifecycle, the checks and the copies are here.  No helper sets
// raft_engine::fork_needed for a write: the entry points differ in that.
#pragma once
#include <initializer_list>

#include "raft_stream.h"

// what raft_audit, raft_monitor and raft_wal begin with: the engine, and one
// device allocation that the handle's pointers are carved from
struct raft_ledger {
    raft_engine* e;
    char* mem;
    size_t bytes;
};

namespace {

// ---- over the eight lanes of a group (observe kernels: 32 groups per
// 256-thread block, lane r < R is replica r; every lane of the wave takes part)
static_assert(RAFT_MAX_R == 8, "eight lanes per group");
__device__ __forceinline__ int32_t group_max(int32_t v) {
#pragma unroll
    for (int d = 1; d < 8; d <<= 1) v = max(v, __shfl_xor(v, d, 64));
    return v;
}
__device__ __forceinline__ long long group_max64(long long v) {
#pragma unroll
    for (int d = 1; d < 8; d <<= 1) v = max(v, __shfl_xor(v, d, 64));
    return v;
}
__device__ __forceinline__ uint32_t group_or(uint32_t v) {
#pragma unroll
    for (int d = 1; d < 8; d <<= 1) v |= __shfl_xor(v, d, 64);
    return v;
}
// the group's byte of a ballot: bit r is its lane r
__device__ __forceinline__ uint32_t group_bits(unsigned long long ballot) {
    return (uint32_t)(ballot >> (threadIdx.x & 56)) & 0xFFu;
}
__device__ __forceinline__ bool differ(int4 a, int4 b) { return a.x != b.x || a.y != b.y || a.z != b.z || a.w != b.w; }

// ---- a handle's lifecycle.  `noun` is what a null handle is called ("null audit")
inline int check_ledger(const raft_ledger* h, int64_t g0, int64_t n, const char* noun) {
    if (!h || !h->e) return raft_internal_fail(RAFT_EINVAL, noun);
    return check_groups(h->e, g0, n);
}
inline int64_t ledger_bytes(const raft_ledger* h) { return h ? (int64_t)h->bytes : 0; }

// the arguments of a create; *out is null from here on
template <class H>
int create_args(raft_engine* e, H** out) {
    if (!e) return raft_internal_fail(RAFT_EINVAL, "null engine");
    if (!out) return raft_internal_fail(RAFT_EINVAL, "null out");
    *out = nullptr;
    return RAFT_OK;
}
// after create_args: a handle H (derived from raft_ledger) with `bytes` of
// device memory, named `what` in a refusal; carve(h) lays the handle's
// pointers into h->mem and brings the tables to their zero state (the handle's
// reset).  The one place a half-made handle is taken apart again.
template <class H, class Carve>
int ledger_create(raft_engine* e, H** out, size_t bytes, const char* what, Carve carve) {
    HIP_TRY(hipSetDevice(e->device));
    H* h = new H{};
    h->e = e;
    int rc;
    if (hipMalloc((void**)&h->mem, bytes) != hipSuccess) {
        h->mem = nullptr;
        rc = raft_internal_fail(RAFT_ENOMEM, std::string(what) + ": hipMalloc failed");
    } else {
        h->bytes = bytes;
        rc = carve(h);
    }
    if (rc != RAFT_OK) {
        (void)hipFree(h->mem);
        delete h;
        return rc;
    }
    *out = h;
    return RAFT_OK;
}
template <class H>
int ledger_destroy(H* h) {
    if (!h) return RAFT_OK;
    if (h->e) {
        (void)hipSetDevice(h->e->device);
        (void)hipStreamSynchronize(h->e->stream);
    }
    (void)hipFree(h->mem);
    delete h;
    return RAFT_OK;
}
// fill(e) enqueues the zero state of every table on the engine stream
template <class Fill>
int ledger_reset(raft_ledger* h, const char* noun, Fill fill) {
    if (int rc = check_ledger(h, 0, 0, noun)) return rc;
    raft_engine* e = h->e;
    HIP_TRY(hipSetDevice(e->device));
    if (int rc = fill(e)) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream));
    return RAFT_OK;
}

// ---- a table's read / write.  The head the accessors share, behind the
// entry point's own check (its result is `checked`): no group is no work, a
// null buffer is refused; body() validates every row of a write, then copies.
template <class Body>
int table_call(int checked, int64_t n, const void* buf, Body body) {
    if (checked) return checked;
    if (n == 0) return RAFT_OK;
    if (!buf) return raft_internal_fail(RAFT_EINVAL, "null buffer");
    return body();
}
// the copy: every region with a host side (a null one is skipped) enqueued on
// the engine stream, then one wait for all of them
struct RowsOut {
    const void* dev;
    void* host;
    size_t bytes;
};
struct RowsIn {
    void* dev;
    const void* host;
    size_t bytes;
};
inline int rows_out(raft_engine* e, std::initializer_list<RowsOut> regions) {
    HIP_TRY(hipSetDevice(e->device));
    for (const RowsOut& r : regions)
        if (r.host) HIP_TRY(hipMemcpyAsync(r.host, r.dev, r.bytes, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return RAFT_OK;
}
inline int rows_out(raft_engine* e, const void* dev, size_t bytes, void* host) { return rows_out(e, {{dev, host, bytes}}); }
// after the caller's validation has passed
inline int rows_in(raft_engine* e, std::initializer_list<RowsIn> regions) {
    HIP_TRY(hipSetDevice(e->device));
    for (const RowsIn& r : regions)
        if (r.host) HIP_TRY(hipMemcpyAsync(r.dev, r.host, r.bytes, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return RAFT_OK;
}
inline int rows_in(raft_engine* e, void* dev, const void* host, size_t bytes) { return rows_in(e, {{dev, host, bytes}}); }

// ---- an observe: eight lanes per group of [g0, g0 + n), the call's counts
// striped at the head of aux.  launch(grid, counts) enqueues the kernel; c
// comes zeroed and holds the folded counts afterwards (zeros when n == 0).
template <class Counts, class Info, class Launch>
int ledger_observe(raft_ledger* h, const char* noun, int64_t g0, int64_t n, Info* info, Counts& c, Launch launch) {
    if (!h || !h->e) return raft_internal_fail(RAFT_EINVAL, noun);
    if (!info) return raft_internal_fail(RAFT_EINVAL, "null info");
    *info = Info{};
    raft_engine* e = h->e;
    if (int rc = check_groups(e, g0, n)) return rc;
    if (n == 0) return RAFT_OK;
    HIP_TRY(hipSetDevice(e->device));
    e->fork_needed = true;                           // later step launches wait for these reads of the state
    if (int rc = raft_internal_grow_dev(e, &e->aux, &e->aux_bytes, Counts::BYTES)) return rc;
    if (int rc = c.zero(e, e->aux)) return rc;
    launch(grid_of(n * 8), c.dev);
    HIP_TRY(hipGetLastError());
    return c.fetch(e);
}

// ---- a listing: the groups of [g0, g0 + n) a source S (raft_stream.h) has a
// record for, at most max_events of them; nothing is consumed.  After the
// range is checked prepare(src) makes the call's own checks and fills the
// source in.  info->delivered, ->pending and ->*total are set.
template <class S, class Info, class Prepare>
int list_records(raft_engine* e, int64_t g0, int64_t n, void* out, int64_t max_events, bool out_on_host, Info* info,
                 int64_t Info::*total, Prepare prepare) {
    if (!info) return raft_internal_fail(RAFT_EINVAL, "null info");
    *info = Info{};
    if (int rc = check_groups(e, g0, n)) return rc;
    S src{};
    if (int rc = prepare(src)) return rc;
    if (int rc = check_records(out, max_events, out_on_host, 16, "max_events")) return rc;
    if (n == 0) return RAFT_OK;
    HIP_TRY(hipSetDevice(e->device));
    e->fork_needed = true;                           // later step launches wait for these reads of the state
    StreamTotals<S> c{};
    const int rc = stream_records(e, src, g0, n, out, max_events, out_on_host, c, &info->delivered);
    info->*total = S::total(c.w);
    info->pending = info->*total - info->delivered;
    return rc;
}
// a handle's report: the listing behind the handle's check, the total in info->flagged
template <class S, class Info, class Prepare>
int ledger_report(raft_ledger* h, const char* noun, int64_t g0, int64_t n, void* out, int64_t max_events,
                  bool out_on_host, Info* info, Prepare prepare) {
    if (!h || !h->e) return raft_internal_fail(RAFT_EINVAL, noun);
    return list_records<S>(h->e, g0, n, out, max_events, out_on_host, info, &Info::flagged, prepare);
}

}  // namespace
