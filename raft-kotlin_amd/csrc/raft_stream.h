// raft_stream.h — internal to the engine library, not installed: what the side
// paths that hand the host an ordered stream of records, cut at a room limit,
// share.  Included by the side-path files only (never by raft_engine.hip: it
// is not one of the step kernel's sources):
//   raft_watch.hip, raft_audit.hip, raft_monitor.hip   a source object each, and the driver
//   raft_apply.hip, raft_outbox.hip   the scan scratch, the record buffer, the publish / the tally
//   raft_fault.hip, raft_snapshot.hip, raft_transfer.hip, raft_noop.hip, raft_sm.hip   the striped tally
// The source-object contract of the flag and write kernels is below and in
// DESIGN.md §4.20.
#pragma once
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include <algorithm>

#include "raft_engine_impl.h"

namespace {

// workgroups of BLOCK threads for n threads
inline unsigned grid_of(int64_t n) { return (unsigned)((n + BLOCK - 1) / BLOCK); }

// ---- the striped tally (DevWords, raft_engine_impl.h): the line of stripe
// (index mod HDR_STRIPES), lines `stride` words apart; index is the wave's
// number in the grid unless the caller counts its waves another way
__device__ __forceinline__ int64_t wave_index() {
    return (int64_t)blockIdx.x * WAVES_PER_BLOCK + (threadIdx.x >> 6);
}
__device__ __forceinline__ unsigned long long* stripe_of(unsigned long long* hdr, int64_t index, int stride = HDR_LINE) {
    return hdr + (index & (HDR_STRIPES - 1)) * stride;
}
// one atomic per nonzero word and wave: called by one lane of the wave
__device__ __forceinline__ void tally(unsigned long long* line, int word, unsigned long long count) {
    if (count) atomicAdd(line + word, count);
}
__device__ __forceinline__ void tally_ballot(unsigned long long* line, int word, unsigned long long ballot) {
    if (ballot) atomicAdd(line + word, (unsigned long long)__popcll(ballot));
}

// ---- the wave-local publish: a wave stages its records in its own slice of
// LDS, then stores the staged words as they lie, lane-strided, so the records
// leave as contiguous stores whatever lane made them.
// The wave's own LDS accesses complete in order: only the compiler must keep
// them so.  No other wave touches the slice, so no workgroup barrier.
__device__ __forceinline__ void wave_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// words [0, words) of st to o; words <= 64 * PER_LANE.  A caller that stages
// again afterwards (a loop) fences once more behind it.
template <int PER_LANE, typename Word>
__device__ __forceinline__ void wave_publish(const Word* st, Word* __restrict__ o, uint32_t words) {
    const uint32_t lane = threadIdx.x & 63;
    wave_lds_fence();
#pragma unroll
    for (int q = 0; q < PER_LANE; ++q) {
        const uint32_t wd = q * 64 + lane;
        if (wd < words) o[wd] = st[wd];
    }
}

// ---- at most one record per group, one group per lane.  A source object S is
// small, trivially copyable and passed by value:
//   S::Word, S::WORDS     a record is WORDS words of Word (uint2 or uint4)
//   S::TALLIES            words of the call's striped totals
//   S::Item               what eval() found; Item::hit: the group has a record
//   Item eval(g, live)    group g; live false (a lane past the range, g clamped): hit is false
//   tallies(it, live, b)  b[k]: the ballot counted into word k (every lane calls it)
//   record(it, g, st)     the record's WORDS words to st
//   commit(it, g)         after the write, in the lane of a group whose record was written
// Pass 1: wcnt[w] = hits among groups [64 w, 64 w + 64) of the range.  An
// exclusive scan of wcnt gives off.  Pass 3: wave w owns those groups and the
// output slots [off[w], off[w] + wcnt[w]), cut at room.  The order of the
// records comes from the scan, never from an atomic; nothing may change what
// eval() sees between the two passes.
template <class S>
__global__ __launch_bounds__(BLOCK) void stream_flag_kernel(S src, int64_t g0, int64_t n, uint32_t* __restrict__ wcnt,
                                                            unsigned long long* hdr) {
    const int64_t j = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const bool live = j < n;
    const int64_t g = g0 + (live ? j : n - 1);                          // g0 <= g < g0 + n <= G (check_groups)
    const typename S::Item it = src.eval(g, live);
    const unsigned long long hits = __ballot(it.hit);
    unsigned long long b[S::TALLIES];
    src.tallies(it, live, b);
    if ((threadIdx.x & 63) == 0 && live) {                              // lane 0 live: the wave is inside the range
        const int64_t wave = wave_index();
        wcnt[wave] = (uint32_t)__popcll(hits);
        unsigned long long* line = stripe_of(hdr, wave);
#pragma unroll
        for (int k = 0; k < S::TALLIES; ++k) tally_ballot(line, k, b[k]);
    }
}

template <class S>
__global__ __launch_bounds__(BLOCK) void stream_write_kernel(S src, int64_t g0, int64_t n,
                                                             const uint32_t* __restrict__ wcnt,
                                                             const unsigned long long* __restrict__ off,
                                                             typename S::Word* __restrict__ out, int64_t max_records) {
    __shared__ typename S::Word stage[WAVES_PER_BLOCK][64 * S::WORDS];  // 64 records per wave
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t wave = wave_index(), j0 = wave * 64;
    if (j0 >= n) return;                                               // wave-uniform
    const uint32_t cnt = wcnt[wave];
    const unsigned long long base = off[wave], room = (unsigned long long)max_records;
    if (cnt == 0 || base >= room) return;                              // wave-uniform: nothing of this wave is written
    const uint32_t take = (uint32_t)min((unsigned long long)cnt, room - base);
    const int64_t j = j0 + lane;
    const bool live = j < n;
    const int64_t g = g0 + (live ? j : n - 1);
    const typename S::Item it = src.eval(g, live);
    // what eval() sees is the flag pass's: the ballot has cnt bits, so every rank is below 64
    const uint32_t rank = (uint32_t)__popcll(__ballot(it.hit) & ((1ull << lane) - 1ull));
    const bool wr = it.hit && rank < take;
    typename S::Word* st = stage[wv];
    if (wr) src.record(it, g, st + S::WORDS * rank);
    wave_publish<S::WORDS>(st, out + base * S::WORDS, S::WORDS * take);  // base + take <= max_records: inside out
    if (wr) src.commit(it, g);
}

// ---- the scan scratch of a stream: [head][counts][offsets][rocprim's], in
// the staging buffer the caller names.  Item is uint32_t (counts, widened to
// 64-bit offsets) or unsigned long long (scanned as it is).
struct CountToOffset {
    __host__ __device__ unsigned long long operator()(uint32_t c) const { return c; }
};
template <typename Item>
struct ScanScratch {
    char* head;
    Item* cnt;
    unsigned long long* off;
    void* tmp;                                       // rocprim's
    size_t items, tmp_bytes = 0;
    static auto input(uint32_t* c) { return rocprim::make_transform_iterator(c, CountToOffset{}); }
    static unsigned long long* input(unsigned long long* c) { return c; }
    int scan_at(raft_engine* e, void* t) {
        HIP_TRY(rocprim::exclusive_scan(t, tmp_bytes, input(t ? cnt : nullptr), t ? off : nullptr, 0ull, items,
                                        rocprim::plus<unsigned long long>(), e->stream));
        return RAFT_OK;
    }
    // size and lay out: *buf grows (grow-only engine staging) to hold head_bytes, the items and the scratch
    int init(raft_engine* e, char** buf, size_t* have, size_t head_bytes, size_t n_items) {
        items = n_items;
        if (int rc = scan_at(e, nullptr)) return rc;
        const size_t cnt_b = al256(items * sizeof(Item)), off_b = al256(items * 8);
        if (int rc = raft_internal_grow_dev(e, buf, have, head_bytes + cnt_b + off_b + al256(tmp_bytes))) return rc;
        head = *buf;
        cnt = (Item*)(head + head_bytes);
        off = (unsigned long long*)(head + head_bytes + cnt_b);
        tmp = head + head_bytes + cnt_b + off_b;
        return RAFT_OK;
    }
    int run(raft_engine* e) { return scan_at(e, tmp); }   // off = exclusive scan of cnt, on the engine stream
};

// ---- the caller's record buffer.  The refusals the streams share: `noun` is
// the room's name in the C-ABI, `align` what the kernels' stores need of a
// device buffer (0: nothing)
inline int check_records(const void* out, int64_t room, bool on_host, unsigned align, const char* noun) {
    if (room < 0) return raft_internal_fail(RAFT_EINVAL, std::string(noun) + " must be >= 0");
    if (!out && room > 0) return raft_internal_fail(RAFT_EINVAL, std::string("null record buffer with ") + noun + " > 0");
    if (!on_host && align && ((uintptr_t)out & (align - 1u)))
        return raft_internal_fail(RAFT_EINVAL, "the record buffer must be " + std::to_string(align) + "-byte aligned");
    return RAFT_OK;
}
// where the kernels write `bytes` of records: the caller's buffer, or apo when
// that is on the host; finish() enqueues the copy back and waits for the stream
struct Records {
    void *user, *dev;
    size_t bytes;
    int begin(raft_engine* e, void* out, size_t n_bytes, bool on_host) {
        user = dev = out;
        bytes = n_bytes;
        if (on_host && bytes > 0) {
            if (int rc = raft_internal_grow_dev(e, &e->apo, &e->apo_bytes, bytes)) return rc;
            dev = e->apo;
        }
        return RAFT_OK;
    }
    int finish(raft_engine* e) {
        if (dev != user) HIP_TRY(hipMemcpyAsync(user, dev, bytes, hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        return RAFT_OK;
    }
};

// ---- the driver of a source: groups [g0, g0 + n), n > 0, at most `room`
// records into out (null: none, a peek).  zero, flag, fetch the totals -- and
// only when something is delivered: scan, write, copy back.  t.w holds the
// call's totals and *delivered the records written, as far as the call got.
// S::total(w) is the number of hits the totals stand for.
template <class S>
using StreamTotals = DevWords<unsigned long long, HDR_STRIPES, HDR_LINE, S::TALLIES, true>;
template <class S>
int stream_records(raft_engine* e, const S& src, int64_t g0, int64_t n, void* out, int64_t room, bool on_host,
                   StreamTotals<S>& t, int64_t* delivered) {
    ScanScratch<uint32_t> sc;
    if (int rc = sc.init(e, &e->aux, &e->aux_bytes, StreamTotals<S>::BYTES, (size_t)((n + 63) / 64))) return rc;
    if (int rc = t.zero(e, sc.head)) return rc;
    const unsigned grid = grid_of(n);
    stream_flag_kernel<S><<<grid, BLOCK, 0, e->stream>>>(src, g0, n, sc.cnt, t.dev);
    HIP_TRY(hipGetLastError());
    if (int rc = t.fetch(e)) return rc;
    *delivered = out ? std::min(S::total(t.w), room) : 0;
    if (*delivered == 0) return RAFT_OK;
    Records rec;
    if (int rc = rec.begin(e, out, (size_t)*delivered * S::WORDS * sizeof(typename S::Word), on_host)) return rc;
    if (int rc = sc.run(e)) return rc;
    stream_write_kernel<S><<<grid, BLOCK, 0, e->stream>>>(src, g0, n, sc.cnt, sc.off, (typename S::Word*)rec.dev, room);
    HIP_TRY(hipGetLastError());
    return rec.finish(e);
}

}  // namespace
