// raft_apply.hip — committed-entry delivery (include/raft_engine.h
// raft_engine_drain_committed*, raft_engine_read_applied / write_applied): the
// reference's lastApplied (RaftServer.kt:47, declared and never used there)
// and the stream of entries that became committed since the last drain.
//
// A separate accessor with kernels of its own: it reads the state words and
// the log rows the step kernel keeps, and writes only its own lastApplied
// array (raft_engine::applied, one int32 per replica, idx = g * R + r) and the
// caller's record buffer.  Three passes on the engine stream:
//   1. count   one thread per selected replica: the committed prefix
//              hi = clamp(min(commitIndex, lastIndex), 0, log_cap) against
//              lo = lastApplied, the ring skip, the regression rule
//   2. scan    exclusive scan of the counts (rocprim): each replica's first
//              output slot; the element past the last replica is the total
//   3. expand  balanced by output slot: a wave owns 64 consecutive replicas
//              and walks their output range 64 slots at a time; each lane
//              finds the replica that owns its slot by a binary search over
//              the wave's offsets (shuffles), reads that 8-byte log slot
//              (lanes inside one run read consecutive slots) and the 24-byte
//              records leave through LDS as contiguous 512-byte stores
// The scan scratch, the record buffer and the publish through LDS are
// raft_stream.h's, shared with the other record streams.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "raft_ledger.h"

using namespace raft;

namespace {

static_assert(sizeof(raft_applied_entry) == 24 && sizeof(raft_drain_info) == 32, "record layouts of the C-ABI");

constexpr int HDR_LOST = 0, HDR_REGRESSED = 1;       // unsigned long long words of the staging header
constexpr size_t HDR_BYTES = 256;

// (the selection, Sel / sel_idx, wave_sum and by_R: raft_engine_impl.h)

// pass 1.  cnt[j]: entries replica j has to deliver, cnt[N] = 0 (the scan's
// last element is then the total).  A drain (not a peek) stores the ring skip
// into lastApplied here, so pass 3 finds lo there.
template <int R>
__global__ __launch_bounds__(BLOCK) void apply_count_kernel(DevParams p, int32_t* __restrict__ applied, Sel s, int peek,
                                                            uint32_t* __restrict__ cnt, unsigned long long* hdr) {
    const int64_t j = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    uint32_t skip = 0, regressed = 0;
    if (j < s.N) {
        const int64_t idx = sel_idx<R>(s, j);
        const int32_t commit = p.st[fidx(p, RAFT_F_COMMIT, idx)];
        const int32_t last = p.st[fidx(p, RAFT_F_LAST, idx)];
        const int32_t hi = committed_hi(p, commit, last);
        int32_t lo = applied[idx];
        if (p.W != FLAT_W) {                                           // a ring: entries below the window are gone
            const int32_t wl = max(0, p.st[fidx(p, RAFT_F_PHYS, idx)] - p.W);
            if (wl > lo && hi > lo) {
                skip = (uint32_t)(min(wl, hi) - lo);
                lo += (int32_t)skip;
                if (!peek) applied[idx] = lo;
            }
        }
        regressed = hi < lo ? 1u : 0u;                                 // lastApplied is monotone: nothing, unchanged
        cnt[j] = hi > lo ? (uint32_t)(hi - lo) : 0u;
    } else if (j == s.N) {
        cnt[j] = 0u;
    }
    // one atomic per wave and word (a skip is < 2^23: a wave's sum fits 32 bits)
    const uint32_t ws = wave_sum(skip), wr = wave_sum(regressed);
    if ((threadIdx.x & 63) == 0) {
        if (ws) atomicAdd(hdr + HDR_LOST, (unsigned long long)ws);
        if (wr) atomicAdd(hdr + HDR_REGRESSED, (unsigned long long)wr);
    }
}

// pass 3.  Wave w of the grid owns replicas [64 w, 64 w + 64) of the selection
// and their output slots [off[64 w], off[64 w + 64)), cut at max_entries.
template <int R>
__global__ __launch_bounds__(BLOCK) void apply_expand_kernel(DevParams p, int32_t* __restrict__ applied, Sel s,
                                                             const uint32_t* __restrict__ cnt,
                                                             const unsigned long long* __restrict__ off,
                                                             uint2* __restrict__ out, int64_t max_entries) {
    __shared__ uint2 stage[WAVES_PER_BLOCK][192];                      // 64 records of 3 words per wave
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t j0 = ((int64_t)blockIdx.x * WAVES_PER_BLOCK + wv) * 64;
    if (j0 >= s.N) return;                                             // wave-uniform
    const int64_t j = j0 + lane;
    const bool mine = j < s.N;
    const int64_t jc = mine ? j : s.N - 1;
    const unsigned long long my_off = mine ? off[j] : off[s.N];
    const uint32_t my_cnt = mine ? cnt[j] : 0u;
    const int64_t my_idx = sel_idx<R>(s, jc);
    const int32_t my_lo = applied[my_idx];
    const unsigned long long base = __shfl(my_off, 0, 64);
    const unsigned long long room = (unsigned long long)max_entries;
    if (base >= room) return;                                          // wave-uniform: no slot left for this tile
    // offsets inside the tile fit 32 bits (64 replicas of < 2^23 slots); the
    // lanes past the selection carry the tile's end, so the search never picks them
    const uint32_t roff = (uint32_t)(my_off - base);
    const uint32_t span = __shfl(roff + my_cnt, 63, 64);
    const uint32_t end = (uint32_t)min((unsigned long long)span, room - base);
    // what a slot's record needs from its owner, fetched by shuffle: lastApplied and
    // (group - the tile's first group, replica) in one word (G < 2^31, at most 64 groups a tile)
    const int32_t g = (int32_t)(my_idx / R);
    const int32_t gw = __shfl(g, 0, 64);
    const int32_t pk = (g - gw) << 3 | (int32_t)(my_idx - (int64_t)g * R);
    constexpr int GPW = 64 / R;
    uint2* st = stage[wv];
    for (uint32_t x0 = 0; x0 < end; x0 += 64) {                        // wave-uniform trip count
        const uint32_t x = x0 + lane;
        const bool live = x < end;
        // owner: the last lane k with roff[k] <= x (its count is then > 0)
        int k = 0;
        uint32_t rk = 0;
#pragma unroll
        for (int step = 32; step > 0; step >>= 1) {
            const uint32_t v = __shfl(roff, k + step, 64);
            const bool take = v <= x;
            k = take ? k + step : k;
            rk = take ? v : rk;
        }
        const int32_t index = __shfl(my_lo, k, 64) + (int32_t)(x - rk);
        const int32_t opk = __shfl(pk, k, 64);
        const int32_t og = gw + (opk >> 3), orr = opk & 7;
        if (live) {
            // the owner's log row (log_of): compile-time R, so no runtime divide
            const int32_t w = og / GPW;
            const uint2* row = p.log + ((int64_t)w * 64 + ((og - w * GPW) * R + orr)) * (int64_t)p.nslots;
            const uint2 e = row[(uint32_t)index & p.wmask];            // index < hi <= log_cap: inside the row
            st[3 * lane + 0] = make_uint2((uint32_t)og, 0u);           // group
            st[3 * lane + 1] = make_uint2((uint32_t)orr, (uint32_t)index);
            st[3 * lane + 2] = e;                                      // (term, cmd) as the log holds them
        }
        wave_publish<3>(st, out + (base + x0) * 3, 3 * min(64u, end - x0));
        wave_lds_fence();                                              // the next trip stages into st again
    }
    // lastApplied moves past what was written, once per replica
    if (mine && my_cnt) {
        const unsigned long long left = my_off < room ? room - my_off : 0ull;
        const uint32_t wrote = (uint32_t)min((unsigned long long)my_cnt, left);
        if (wrote) applied[my_idx] = my_lo + (int32_t)wrote;
    }
}

template <int R> struct CountL {
    static void run(raft_engine* e, const Sel& s, int peek, uint32_t* cnt, unsigned long long* hdr) {
        const unsigned grid = grid_of(s.N + 1);
        apply_count_kernel<R><<<grid, BLOCK, 0, e->stream>>>(e->dp, e->applied, s, peek, cnt, hdr);
    }
};
template <int R> struct ExpandL {
    static void run(raft_engine* e, const Sel& s, const uint32_t* cnt, const unsigned long long* off, uint2* out,
                    int64_t max_entries) {
        const int64_t tiles = (s.N + 63) / 64;
        const unsigned grid = (unsigned)((tiles + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK);
        apply_expand_kernel<R><<<grid, BLOCK, 0, e->stream>>>(e->dp, e->applied, s, cnt, off, out, max_entries);
    }
};

int mark(raft_engine* e, int k) {                   // a pass boundary of a timed drain
    if (!e->drain_timing) return RAFT_OK;
    HIP_TRY(hipEventRecord(e->ev_drain[k], e->stream));
    return RAFT_OK;
}

int drain(raft_engine* e, int64_t g0, int64_t n, int32_t replica, raft_applied_entry* out, int64_t max_entries,
          raft_drain_info* info, bool out_on_host) {
    if (!e) return raft_internal_fail(RAFT_EINVAL, "null engine");
    if (!info) return raft_internal_fail(RAFT_EINVAL, "null info");
    if (int rc = check_groups(e, g0, n)) return rc;
    if (replica < -1 || replica >= e->p.R) return raft_internal_fail(RAFT_EINVAL, "replica must be -1 or in 0..R-1");
    if (int rc = check_records(out, max_entries, out_on_host, 0, "max_entries")) return rc;
    *info = raft_drain_info{0, 0, 0, 0};
    if (n == 0) return RAFT_OK;
    const bool peek = !out && max_entries == 0;
    HIP_TRY(hipSetDevice(e->device));
    e->fork_needed = true;                           // later step launches wait for these reads of the state and logs
    const Sel s{g0, replica < 0 ? n * e->p.R : n, replica};
    ScanScratch<uint32_t> sc;                        // one item per selected replica and the zero behind them
    if (int rc = sc.init(e, &e->apl, &e->apl_bytes, HDR_BYTES, (size_t)s.N + 1)) return rc;
    unsigned long long* hdr = (unsigned long long*)sc.head;

    if (int rc = mark(e, 0)) return rc;
    HIP_TRY(hipMemsetAsync(hdr, 0, HDR_BYTES, e->stream));
    by_R<CountL>(e->p.R, e, s, peek ? 1 : 0, sc.cnt, hdr);
    HIP_TRY(hipGetLastError());
    if (int rc = mark(e, 1)) return rc;
    if (int rc = sc.run(e)) return rc;
    if (int rc = mark(e, 2)) return rc;
    unsigned long long h[2] = {0, 0}, total = 0;
    HIP_TRY(hipMemcpyAsync(h, hdr, sizeof(h), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipMemcpyAsync(&total, sc.off + s.N, 8, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    const int64_t delivered = peek ? 0 : std::min<int64_t>((int64_t)total, max_entries);
    info->delivered = delivered;
    info->pending = (int64_t)total - delivered;
    info->lost = (int64_t)h[HDR_LOST];
    info->regressed = (int64_t)h[HDR_REGRESSED];
    if (delivered > 0) {
        Records rec;
        if (int rc = rec.begin(e, out, (size_t)delivered * sizeof(raft_applied_entry), out_on_host)) return rc;
        if (int rc = mark(e, 3)) return rc;
        by_R<ExpandL>(e->p.R, e, s, sc.cnt, sc.off, (uint2*)rec.dev, max_entries);
        HIP_TRY(hipGetLastError());
        if (int rc = mark(e, 4)) return rc;
        if (int rc = rec.finish(e)) return rc;
    }
    e->drain_expanded = delivered > 0;
    if (info->lost > 0)
        return raft_internal_fail(RAFT_EWINDOW, std::to_string(info->lost) +
                                                    " committed entries left the log window undelivered (skipped)");
    return RAFT_OK;
}

}  // namespace

extern "C" {

int raft_engine_drain_committed(raft_engine* e, int64_t g0, int64_t n, int32_t replica, raft_applied_entry* out_host,
                                int64_t max_entries, raft_drain_info* info) {
    return drain(e, g0, n, replica, out_host, max_entries, info, true);
}

int raft_engine_drain_committed_dev(raft_engine* e, int64_t g0, int64_t n, int32_t replica, raft_applied_entry* out_dev,
                                    int64_t max_entries, raft_drain_info* info) {
    return drain(e, g0, n, replica, out_dev, max_entries, info, false);
}

// replicas are indexed g * R + r: a range of groups is one contiguous run of lastApplied
int raft_engine_read_applied(raft_engine* e, int64_t g0, int64_t n, int32_t* out) {
    return table_call(check_groups(e, g0, n), n, out,
                      [&] { return rows_out(e, e->applied + g0 * e->p.R, (size_t)n * e->p.R * 4, out); });
}

int raft_engine_write_applied(raft_engine* e, int64_t g0, int64_t n, const int32_t* in) {
    return table_call(check_groups(e, g0, n), n, in, [&]() -> int {
        for (int64_t k = 0; k < n * e->p.R; ++k)     // a drain reads log slots [lastApplied, hi): keep it inside the row
            if (in[k] < 0 || in[k] > e->p.log_cap)
                return raft_internal_fail(RAFT_EINVAL, "lastApplied must be in 0..log_cap");
        return rows_in(e, e->applied + g0 * e->p.R, in, (size_t)n * e->p.R * 4);
    });
}

// Not in the header (scripts/drain_probe.py): while enabled, a drain records an
// event at each pass boundary; ms[3] = count, scan, expand of the last drain
// (the host's read of the totals between scan and expand is not in them;
// expand is 0 when nothing was delivered).
int raft_internal_drain_timing(raft_engine* e, int enable) {
    if (!e) return raft_internal_fail(RAFT_EINVAL, "null engine");
    HIP_TRY(hipSetDevice(e->device));
    for (hipEvent_t& x : e->ev_drain)
        if (enable && !x) HIP_TRY(hipEventCreate(&x));
    e->drain_timing = enable != 0;
    return RAFT_OK;
}

int raft_internal_drain_pass_ms(raft_engine* e, double* ms) {
    if (!e || !ms || !e->drain_timing) return raft_internal_fail(RAFT_EINVAL, "drain timing is off");
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipStreamSynchronize(e->stream));
    for (int k = 0; k < 3; ++k) {
        float f = 0.f;
        const int a = k < 2 ? k : 3;
        if (k < 2 || e->drain_expanded) HIP_TRY(hipEventElapsedTime(&f, e->ev_drain[a], e->ev_drain[a + 1]));
        ms[k] = f;
    }
    return RAFT_OK;
}

}  // extern "C"
