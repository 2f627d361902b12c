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
//              against seen[g]; a ballot / popcount per wave gives the wave's
//              number of changed groups, and the kind counts go into the
//              wave's stripe (one atomic per nonzero word and wave)
//   2. scan    exclusive scan of the per-wave counts (rocprim): n / 64 items.
//              The order of the records comes from it, never from an atomic.
//   3. write   each wave that has changed groups below the cut evaluates its
//              groups again, ranks its changed lanes by the ballot below the
//              lane, sends the records through LDS as contiguous stores and
//              stores seen for the lanes it wrote
// Passes 2 and 3 run only when something is delivered: a poll that finds
// nothing changed is one memset, one kernel and one 4-KB copy.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include <algorithm>
#include <string>

#include "raft_engine_impl.h"

using namespace raft;

namespace {

static_assert(sizeof(raft_leader_event) == 24 && sizeof(raft_watch_info) == 64, "record layouts of the C-ABI");

// the counts of a call, striped as a restart's totals, at the head of aux
enum { WW_GAINED = 0, WW_LOST = 1, WW_MOVED = 2, WW_RETERM = 3, WW_LEADERLESS = 4, WW_WORDS = 5 };
using Counts = DevWords<unsigned long long, HDR_STRIPES, HDR_LINE, WW_WORDS, true>;

// a group's current (leader, term) and what the watch last reported for it
struct Watch {
    int2 cur, seen;
    bool changed;
};
__device__ __forceinline__ Watch watch_of(const DevParams& p, const int2* __restrict__ seen, int64_t g, bool live) {
    const Lead l = find_newest_leader(p, g);
    Watch w;
    w.cur = l.r >= 0 ? make_int2(l.r, l.term) : make_int2(-1, 0);
    w.seen = seen[g];
    w.changed = live && (w.cur.x != w.seen.x || w.cur.y != w.seen.y);
    return w;
}

__global__ __launch_bounds__(BLOCK) void watch_fill_kernel(int2* __restrict__ seen, int64_t G) {
    const int64_t g = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (g < G) seen[g] = make_int2(-1, 0);
}

// pass 1.  wcnt[w]: changed groups among groups [64 w, 64 w + 64) of the range
__global__ __launch_bounds__(BLOCK) void watch_flag_kernel(DevParams p, const int2* __restrict__ seen, int64_t g0,
                                                           int64_t n, uint32_t* __restrict__ wcnt,
                                                           unsigned long long* hdr) {
    const int64_t j = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const bool live = j < n;
    const int64_t g = g0 + (live ? j : n - 1);                          // g0 <= g < g0 + n <= G (check_groups)
    const Watch w = watch_of(p, seen, g, live);
    const bool gained = w.changed && w.seen.x < 0 && w.cur.x >= 0, lost = w.changed && w.seen.x >= 0 && w.cur.x < 0,
               moved = w.changed && w.seen.x >= 0 && w.cur.x >= 0 && w.seen.x != w.cur.x;
    const unsigned long long b_chg = __ballot(w.changed), b_gain = __ballot(gained), b_lost = __ballot(lost),
                             b_mov = __ballot(moved), b_ret = __ballot(w.changed && !gained && !lost && !moved),
                             b_none = __ballot(live && w.cur.x < 0);
    if ((threadIdx.x & 63) == 0 && live) {                              // lane 0 live: the wave is inside the range
        const int64_t wave = (int64_t)blockIdx.x * WAVES_PER_BLOCK + (threadIdx.x >> 6);
        wcnt[wave] = (uint32_t)__popcll(b_chg);
        unsigned long long* line = hdr + (wave & (HDR_STRIPES - 1)) * HDR_LINE;
        if (b_gain) atomicAdd(line + WW_GAINED, (unsigned long long)__popcll(b_gain));
        if (b_lost) atomicAdd(line + WW_LOST, (unsigned long long)__popcll(b_lost));
        if (b_mov) atomicAdd(line + WW_MOVED, (unsigned long long)__popcll(b_mov));
        if (b_ret) atomicAdd(line + WW_RETERM, (unsigned long long)__popcll(b_ret));
        if (b_none) atomicAdd(line + WW_LEADERLESS, (unsigned long long)__popcll(b_none));
    }
}

struct CountToOffset {
    __host__ __device__ unsigned long long operator()(uint32_t c) const { return c; }
};

// pass 3.  Wave w owns groups [64 w, 64 w + 64) of the range and the output
// slots [off[w], off[w] + wcnt[w]), cut at max_events.
__global__ __launch_bounds__(BLOCK) void watch_write_kernel(DevParams p, int2* __restrict__ seen, int64_t g0, int64_t n,
                                                            const uint32_t* __restrict__ wcnt,
                                                            const unsigned long long* __restrict__ off,
                                                            uint2* __restrict__ out, int64_t max_events) {
    __shared__ uint2 stage[WAVES_PER_BLOCK][192];                      // 64 records of 3 words per wave
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t wave = (int64_t)blockIdx.x * WAVES_PER_BLOCK + wv;
    const int64_t j0 = wave * 64;
    if (j0 >= n) return;                                               // wave-uniform
    const uint32_t cnt = wcnt[wave];
    const unsigned long long base = off[wave], room = (unsigned long long)max_events;
    if (cnt == 0 || base >= room) return;                              // wave-uniform: nothing of this wave is written
    const uint32_t take = (uint32_t)min((unsigned long long)cnt, room - base);
    const int64_t j = j0 + lane;
    const bool live = j < n;
    const int64_t g = g0 + (live ? j : n - 1);
    const Watch w = watch_of(p, seen, g, live);
    // the state is the flag pass's: the ballot has cnt bits, so every rank is below 64
    const uint32_t rank = (uint32_t)__popcll(__ballot(w.changed) & ((1ull << lane) - 1ull));
    const bool wr = w.changed && rank < take;
    uint2* st = stage[wv];
    if (wr) {
        st[3 * rank + 0] = make_uint2((uint32_t)((uint64_t)g & 0xFFFFFFFFu), (uint32_t)((uint64_t)g >> 32));
        st[3 * rank + 1] = make_uint2((uint32_t)w.cur.x, (uint32_t)w.cur.y);
        st[3 * rank + 2] = make_uint2((uint32_t)w.seen.x, (uint32_t)w.seen.y);
    }
    // the wave's own LDS accesses complete in order: only the compiler must keep them so
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const uint32_t words = 3 * take;                                   // base + take <= max_events: inside out
    uint2* o = out + base * 3;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const uint32_t wd = q * 64 + lane;
        if (wd < words) o[wd] = st[wd];
    }
    if (wr) seen[g] = w.cur;                                           // reported: the group's lane owns the pair
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
    if (max_events < 0) return raft_internal_fail(RAFT_EINVAL, "max_events must be >= 0");
    if (!out && max_events > 0) return raft_internal_fail(RAFT_EINVAL, "null record buffer with max_events > 0");
    if (!out_on_host && ((uintptr_t)out & 7u))
        return raft_internal_fail(RAFT_EINVAL, "the record buffer must be 8-byte aligned");
    if (n == 0) return RAFT_OK;
    const bool peek = !out && max_events == 0;
    HIP_TRY(hipSetDevice(e->device));
    e->fork_needed = true;                           // later step launches wait for these reads of the state
    if (int rc = ensure_watch(e)) return rc;
    const size_t nwaves = (size_t)((n + 63) / 64);
    const auto counts_of = [](uint32_t* c) { return rocprim::make_transform_iterator(c, CountToOffset{}); };
    size_t scan_b = 0;
    HIP_TRY(rocprim::exclusive_scan(nullptr, scan_b, counts_of(nullptr), (unsigned long long*)nullptr, 0ull, nwaves,
                                    rocprim::plus<unsigned long long>(), e->stream));
    const size_t cnt_b = al256(nwaves * 4), off_b = al256(nwaves * 8);
    if (int rc = raft_internal_grow_dev(e, &e->aux, &e->aux_bytes, Counts::BYTES + cnt_b + off_b + al256(scan_b)))
        return rc;
    uint32_t* wcnt = (uint32_t*)(e->aux + Counts::BYTES);
    unsigned long long* off = (unsigned long long*)(e->aux + Counts::BYTES + cnt_b);
    void* scan_tmp = e->aux + Counts::BYTES + cnt_b + off_b;
    Counts c;
    if (int rc = c.zero(e, e->aux)) return rc;
    const unsigned grid = (unsigned)((n + BLOCK - 1) / BLOCK);
    watch_flag_kernel<<<grid, BLOCK, 0, e->stream>>>(e->dp, e->watch, g0, n, wcnt, c.dev);
    HIP_TRY(hipGetLastError());
    if (int rc = c.fetch(e)) return rc;
    const int64_t total = (int64_t)(c.w[WW_GAINED] + c.w[WW_LOST] + c.w[WW_MOVED] + c.w[WW_RETERM]);
    const int64_t delivered = peek ? 0 : std::min(total, max_events);
    info->delivered = delivered;
    info->pending = total - delivered;
    info->gained = (int64_t)c.w[WW_GAINED];
    info->lost = (int64_t)c.w[WW_LOST];
    info->moved = (int64_t)c.w[WW_MOVED];
    info->reterm = (int64_t)c.w[WW_RETERM];
    info->leaderless = (int64_t)c.w[WW_LEADERLESS];
    if (delivered == 0) return RAFT_OK;
    uint2* dst = (uint2*)out;
    if (out_on_host) {
        if (int rc = raft_internal_grow_dev(e, &e->apo, &e->apo_bytes, (size_t)delivered * sizeof(raft_leader_event)))
            return rc;
        dst = (uint2*)e->apo;
    }
    HIP_TRY(rocprim::exclusive_scan(scan_tmp, scan_b, counts_of(wcnt), off, 0ull, nwaves,
                                    rocprim::plus<unsigned long long>(), e->stream));
    HIP_TRY(hipGetLastError());
    watch_write_kernel<<<grid, BLOCK, 0, e->stream>>>(e->dp, e->watch, g0, n, wcnt, off, dst, max_events);
    HIP_TRY(hipGetLastError());
    if (out_on_host)
        HIP_TRY(hipMemcpyAsync(out, dst, (size_t)delivered * sizeof(raft_leader_event), hipMemcpyDeviceToHost,
                               e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return RAFT_OK;
}

}  // namespace

// raft_outbox.hip: a proposal outbox configured behind the seen pairs (it shares this allocation) is emptied
int raft_internal_outbox_reset(raft_engine* e);

// raft_engine_reset, and the first use: nothing reported yet
int raft_internal_watch_reset(raft_engine* e) {
    if (!e->watch) return RAFT_OK;
    if (int rc = raft_internal_outbox_reset(e)) return rc;
    const unsigned grid = (unsigned)((e->p.G + BLOCK - 1) / BLOCK);
    watch_fill_kernel<<<grid, BLOCK, 0, e->stream>>>(e->watch, e->p.G);
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

int raft_engine_read_watch(raft_engine* e, int64_t g0, int64_t n, int32_t* out) {
    if (int rc = check_groups(e, g0, n)) return rc;
    if (n == 0) return RAFT_OK;
    if (!out) return raft_internal_fail(RAFT_EINVAL, "null buffer");
    HIP_TRY(hipSetDevice(e->device));
    if (int rc = ensure_watch(e)) return rc;
    HIP_TRY(hipMemcpyAsync(out, e->watch + g0, (size_t)n * sizeof(int2), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return RAFT_OK;
}

int raft_engine_write_watch(raft_engine* e, int64_t g0, int64_t n, const int32_t* in) {
    if (int rc = check_groups(e, g0, n)) return rc;
    if (n == 0) return RAFT_OK;
    if (!in) return raft_internal_fail(RAFT_EINVAL, "null buffer");
    for (int64_t k = 0; k < n; ++k) {
        const int32_t leader = in[2 * k], term = in[2 * k + 1];
        if (leader < -1 || leader >= e->p.R || term < 0 || (leader < 0 && term != 0))
            return raft_internal_fail(RAFT_EINVAL, "a watch pair is (-1, 0) or (leader in 0..R-1, term >= 0)");
    }
    HIP_TRY(hipSetDevice(e->device));
    if (int rc = ensure_watch(e)) return rc;
    HIP_TRY(hipMemcpyAsync(e->watch + g0, in, (size_t)n * sizeof(int2), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return RAFT_OK;
}

}  // extern "C"
