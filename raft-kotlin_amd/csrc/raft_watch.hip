// raft_watch.hip — the leader watch (include/raft_engine.h
// raft_engine_poll_leaders*, raft_engine_read_watch / write_watch): the groups
// whose newest leader or its term changed since the watch last reported them,
// as a stream of 24-byte records in ascending group order.  What etcd hands out
// as SoftState in a Ready and TiKV through its role observer; the reference has
// no counterpart.
//
// A side path between two step launches with kernels of its own: it reads the
// R role / term words of each group (quad 0 of each replica, load_roles) and
// writes only its own `seen` array (raft_engine::watch, one (leader, term) pair
// per group, never part of the state export or the digest) and the caller's
// record buffer.  A stream compaction over groups, on the engine stream:
//   1. flag    one thread per group: the newest leader (find_newest_leader)
//              against seen[g]; the wave's number of changed groups and the
//              kind counts
//   2. scan    of the per-wave counts
//   3. write   the records of the waves below the cut, then seen for the
//              groups written
// The three passes, their kernels and their host side are raft_stream.h's
// (DESIGN.md §4.20); this file holds the watch's source object.  Passes 2 and
// 3 run only when something is delivered: a poll that finds nothing changed is
// one memset, one kernel and one 4-KB copy.
#include <hip/hip_runtime.h>

#include <string>

#include "raft_ledger.h"

using namespace raft;

namespace {

static_assert(sizeof(raft_leader_event) == 24 && sizeof(raft_watch_info) == 64, "record layouts of the C-ABI");

// the counts of a call, striped as a restart's totals, at the head of aux
enum { WW_GAINED = 0, WW_LOST = 1, WW_MOVED = 2, WW_RETERM = 3, WW_LEADERLESS = 4, WW_WORDS = 5 };

// the stream's source: a group's current (leader, term) against what the watch last reported for it
struct WatchSource {
    using Word = uint2;
    static constexpr int WORDS = 3, TALLIES = WW_WORDS;
    struct Item {
        int2 cur, seen;
        bool hit;                                                       // changed
    };
    DevParams p;
    int2* __restrict__ seen;

    __device__ __forceinline__ Item eval(int64_t g, bool live) const {
        const Lead l = find_newest_leader(p, g);
        const int2 cur = l.r >= 0 ? make_int2(l.r, l.term) : make_int2(-1, 0), was = seen[g];
        return Item{cur, was, live && (cur.x != was.x || cur.y != was.y)};
    }
    __device__ __forceinline__ void tallies(const Item& w, bool live, unsigned long long (&b)[TALLIES]) const {
        const bool gained = w.hit && w.seen.x < 0 && w.cur.x >= 0, lost = w.hit && w.seen.x >= 0 && w.cur.x < 0,
                   moved = w.hit && w.seen.x >= 0 && w.cur.x >= 0 && w.seen.x != w.cur.x;
        b[WW_GAINED] = __ballot(gained);
        b[WW_LOST] = __ballot(lost);
        b[WW_MOVED] = __ballot(moved);
        b[WW_RETERM] = __ballot(w.hit && !gained && !lost && !moved);
        b[WW_LEADERLESS] = __ballot(live && w.cur.x < 0);
    }
    __device__ __forceinline__ void record(const Item& w, int64_t g, uint2* st) const {
        st[0] = make_uint2((uint32_t)((uint64_t)g & 0xFFFFFFFFu), (uint32_t)((uint64_t)g >> 32));
        st[1] = make_uint2((uint32_t)w.cur.x, (uint32_t)w.cur.y);
        st[2] = make_uint2((uint32_t)w.seen.x, (uint32_t)w.seen.y);
    }
    __device__ __forceinline__ void commit(const Item& w, int64_t g) const { seen[g] = w.cur; }   // reported: the lane owns the pair
    static int64_t total(const unsigned long long* w) {
        return (int64_t)(w[WW_GAINED] + w[WW_LOST] + w[WW_MOVED] + w[WW_RETERM]);
    }
};

__global__ __launch_bounds__(BLOCK) void watch_fill_kernel(int2* __restrict__ seen, int64_t G) {
    const int64_t g = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (g < G) seen[g] = make_int2(-1, 0);
}

// seen: allocated and set to (-1, 0) at the first call that needs it
int ensure_watch(raft_engine* e) {
    if (e->watch) return RAFT_OK;
    const size_t bytes = al256((size_t)e->p.G * sizeof(int2));
    HIP_TRY(hipMalloc((void**)&e->watch, bytes));
    e->watch_bytes = bytes;
    return raft_internal_watch_reset(e);
}

int poll(raft_engine* e, int64_t g0, int64_t n, raft_leader_event* out, int64_t max_events, raft_watch_info* info,
         bool out_on_host) {
    if (!e) return raft_internal_fail(RAFT_EINVAL, "null engine");
    if (!info) return raft_internal_fail(RAFT_EINVAL, "null info");
    *info = raft_watch_info{};
    if (int rc = check_groups(e, g0, n)) return rc;
    if (int rc = check_records(out, max_events, out_on_host, 8, "max_events")) return rc;
    if (n == 0) return RAFT_OK;
    HIP_TRY(hipSetDevice(e->device));
    e->fork_needed = true;                           // later step launches wait for these reads of the state
    if (int rc = ensure_watch(e)) return rc;
    StreamTotals<WatchSource> c{};
    const int rc = stream_records(e, WatchSource{e->dp, e->watch}, g0, n, out, max_events, out_on_host, c, &info->delivered);
    info->pending = WatchSource::total(c.w) - info->delivered;
    info->gained = (int64_t)c.w[WW_GAINED];
    info->lost = (int64_t)c.w[WW_LOST];
    info->moved = (int64_t)c.w[WW_MOVED];
    info->reterm = (int64_t)c.w[WW_RETERM];
    info->leaderless = (int64_t)c.w[WW_LEADERLESS];
    return rc;
}

}  // namespace

// raft_outbox.hip: a proposal outbox configured behind the seen pairs (it shares this allocation) is emptied
int raft_internal_outbox_reset(raft_engine* e);

// raft_engine_reset, and the first use: nothing reported yet
int raft_internal_watch_reset(raft_engine* e) {
    if (!e->watch) return RAFT_OK;
    if (int rc = raft_internal_outbox_reset(e)) return rc;
    watch_fill_kernel<<<grid_of(e->p.G), BLOCK, 0, e->stream>>>(e->watch, e->p.G);
    HIP_TRY(hipGetLastError());
    return RAFT_OK;
}

extern "C" {

int raft_engine_poll_leaders(raft_engine* e, int64_t g0, int64_t n, raft_leader_event* out_host, int64_t max_events,
                             raft_watch_info* info) {
    return poll(e, g0, n, out_host, max_events, info, true);
}

int raft_engine_poll_leaders_dev(raft_engine* e, int64_t g0, int64_t n, raft_leader_event* out_dev, int64_t max_events,
                                 raft_watch_info* info) {
    return poll(e, g0, n, out_dev, max_events, info, false);
}

// the pairs are allocated at the first call that needs them: before the copy, on the engine's device
int raft_engine_read_watch(raft_engine* e, int64_t g0, int64_t n, int32_t* out) {
    return table_call(check_groups(e, g0, n), n, out, [&]() -> int {
        HIP_TRY(hipSetDevice(e->device));
        if (int rc = ensure_watch(e)) return rc;
        return rows_out(e, e->watch + g0, (size_t)n * sizeof(int2), out);
    });
}

int raft_engine_write_watch(raft_engine* e, int64_t g0, int64_t n, const int32_t* in) {
    return table_call(check_groups(e, g0, n), n, in, [&]() -> int {
        for (int64_t k = 0; k < n; ++k) {
            const int32_t leader = in[2 * k], term = in[2 * k + 1];
            if (leader < -1 || leader >= e->p.R || term < 0 || (leader < 0 && term != 0))
                return raft_internal_fail(RAFT_EINVAL, "a watch pair is (-1, 0) or (leader in 0..R-1, term >= 0)");
        }
        HIP_TRY(hipSetDevice(e->device));
        if (int rc = ensure_watch(e)) return rc;
        return rows_in(e, e->watch + g0, in, (size_t)n * sizeof(int2));
    });
}

}  // extern "C"
