// raft_engine_impl.h — internal to the engine library, not installed: what its
// translation units share.
//   raft_engine.hip   the step kernel, the accessors, the C-ABI
//   raft_batch.hip    the handler batches (include/raft_engine.h raft_*_batch*)
//   raft_apply.hip    the committed-entry drain
//   raft_client.hip   the leader directory, routed proposals and tickets
//   raft_sm.hip       the replicated state machine
//   raft_fault.hip    replica restart
//   raft_read.hip     linearizable reads
//   raft_snapshot.hip snapshot install
//   raft_transfer.hip leadership transfer
//   raft_noop.hip     leader no-op entries
//   raft_watch.hip    the leader watch
// Device side: the HBM indexing helpers, a replica's quad load / store, the
// leader lookups, the committed prefix.  Host side: the engine object and the
// call plumbing of the entry points -- HIP_TRY, the argument checks, the
// staging of a host call's arrays (Staged), the readback of a call's status
// words or totals (DevWords).
#pragma once
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort_config.hpp>

#include <cstring>
#include <string>
#include <vector>

#include "raft_step.h"

using namespace raft;

// raft_engine.hip: set raft_last_error() and return `code`; grow-only engine
// staging (device / page-locked host), kept for the engine's lifetime
int raft_internal_fail(int code, const std::string& msg);
extern "C" int raft_internal_grow_dev(raft_engine* e, char** buf, size_t* have, size_t need);
extern "C" int raft_internal_grow_host(raft_engine* e, char** buf, size_t* have, size_t need);
// raft_engine.hip: enqueue the log-tail cache's rebuild on the engine stream
// if a host write left it stale (cache_valid false)
void raft_internal_ensure_cache(raft_engine* e);
// raft_watch.hip: enqueue "nothing reported yet" for the leader watch on the
// engine stream, if the watch is allocated (raft_engine_reset)
int raft_internal_watch_reset(raft_engine* e);

#define HIP_TRY(expr)                                                                                    \
    do {                                                                                                 \
        hipError_t _e = (expr);                                                                          \
        if (_e != hipSuccess)                                                                            \
            return raft_internal_fail(RAFT_EDEVICE, std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)

// rocprim's radix sort takes its merge-sort path up to 2^20 items (one
// block sort and ~10 merge passes over the whole array, 21 dispatches at 10^6
// messages); a merge limit of 0 keeps it on the onesweep path (a histogram
// pass and one pass per 8 key bits).
using SortConfig = rocprim::radix_sort_config<rocprim::default_config, rocprim::default_config,
                                              rocprim::default_config, 0>;

namespace {

constexpr int BLOCK = 256;
constexpr int WAVES_PER_BLOCK = BLOCK / 64;

inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// field f of replica idx = g * R + r in the state quads (DevParams::st,
// raft_step.h FIELD_SLOT): word f & 3 of quad f >> 2 of the replica's slots
__device__ __forceinline__ int64_t fidx(const DevParams& p, int f, int64_t idx) {
    const int s = FIELD_SLOT[f];
    return ((int64_t)(s >> 2) * p.GR + idx) * 4 + (s & 3);
}
// quad q of replica idx (16-B aligned: the state array starts on 256 B)
__device__ __forceinline__ int4* quad(const DevParams& p, int q, int64_t idx) {
    return (int4*)p.st + (int64_t)q * p.GR + idx;
}

// the log of replica idx = g * R + r outside the step kernel: lane
// (g % GPW) * R + r of the block of step-kernel wave g / GPW
__device__ __forceinline__ LogView log_of(const DevParams& p, int64_t idx) {
    const int64_t g = idx / p.R;
    const int gpw = 64 / p.R;
    const int64_t w = g / gpw;
    const int lane = (int)(g - w * gpw) * p.R + (int)(idx - g * p.R);
    return LogView{p.log + (w * 64 + lane) * (int64_t)p.nslots, (uint32_t)p.nslots, p.wmask, p.cap, p.W};
}

// the committed prefix of a replica, in entries: min(commitIndex, lastIndex) within 0..log_cap
__device__ __forceinline__ int32_t committed_hi(const DevParams& p, int32_t commit, int32_t last) {
    return max(0, min(min(commit, last), p.cap));
}

// ---- one replica in registers: the handler batches (raft_batch.hip) and the
// routed proposals (raft_client.hip) load, change and store it the same way
struct RepState {
    int32_t term, voted, role, commit, last, phys, elec, phase, retry;
    uint32_t fl;
    int32_t t1, t2;
    uint32_t c1;
    __device__ Rep ref() { return Rep{term, voted, role, commit, last, phys, elec, phase, retry, fl, t1, t2, c1}; }
};

// The replica's state quads a handler needs (raft_step.h FIELD_SLOT), one
// 16-B access and one 32-B sector each: quad 0 (term, votedFor, state, flags)
// and quad 1 (lastIndex, physLen, t1, electionMs) for vote() and the timer
// re-arm (RaftServer.kt:228-251); quad 2 (commitIndex, t2, c1, phaseMs) too
// for append() and appendCommand (:253-287, :100-107).  Quad 3 (retryMs and
// the primary session) no handler touches.  The log-tail cache (t1, t2, c1)
// is the HBM copy: the batch path keeps it valid (run_batch_dev rebuilds it
// first when a host write left it stale, and every run stores it back), so
// vote() reads no log slot at all.
struct RepQuads {
    int4 q0, q1, q2;
};
template <bool VOTE_ONLY = false>
__device__ __forceinline__ void load_rep(RepState& x, RepQuads& o, const DevParams& p, int64_t idx) {
    o.q0 = *quad(p, 0, idx);
    o.q1 = *quad(p, 1, idx);
    o.q2 = VOTE_ONLY ? make_int4(0, 0, 0, 0) : *quad(p, 2, idx);
    x.term = o.q0.x; x.voted = o.q0.y; x.role = o.q0.z; x.fl = (uint32_t)o.q0.w;
    x.last = o.q1.x; x.phys = o.q1.y; x.t1 = o.q1.z; x.elec = o.q1.w;
    x.commit = o.q2.x; x.t2 = o.q2.y; x.c1 = (uint32_t)o.q2.z; x.phase = o.q2.w;
    x.retry = 0;                                                        // (quad 3: no handler touches it)
}

// Only the quads that changed are written back, whole (the run's thread owns
// the replica): a random replica's quad is a 32-B sector of its own.
template <bool VOTE_ONLY = false>
__device__ __forceinline__ void store_rep(const RepState& x, const RepQuads& o, const DevParams& p, int64_t idx) {
    const int4 q0 = make_int4(x.term, x.voted, x.role, (int32_t)(x.fl & FL_EXPORT_MASK));
    const int4 q1 = make_int4(x.last, x.phys, x.t1, x.elec);
    const int4 q2 = make_int4(x.commit, x.t2, (int32_t)x.c1, x.phase);
    auto differ = [](int4 a, int4 b) { return a.x != b.x || a.y != b.y || a.z != b.z || a.w != b.w; };
    if (differ(q0, o.q0)) *quad(p, 0, idx) = q0;
    if (differ(q1, o.q1)) *quad(p, 1, idx) = q1;
    if (!VOTE_ONLY && differ(q2, o.q2)) *quad(p, 2, idx) = q2;
}

// The R role words of group g: reads of quad 0 (which also holds currentTerm),
// all R in flight at once: unconditional loads at a clamped index, as
// bucket_tile_kernel's.  q[r] is replica r's for r < R.
__device__ __forceinline__ void load_roles(const DevParams& p, int64_t g, int4 (&q)[RAFT_MAX_R]) {
    const int R = p.R;
    const int4* q0 = quad(p, 0, g * R);
#pragma unroll
    for (int r = 0; r < RAFT_MAX_R; ++r) q[r] = q0[min(r, R - 1)];
}

// The group's leader as RAFT_CMD_LOWEST_LEADER chooses it: the lowest replica
// index whose role is LEADER.
struct Lead {
    int32_t r, n, term;
};
__device__ __forceinline__ Lead find_leader(const DevParams& p, int64_t g) {
    int4 q[RAFT_MAX_R];
    load_roles(p, g, q);
    const int R = p.R;
    Lead l{-1, 0, 0};
#pragma unroll
    for (int r = RAFT_MAX_R - 1; r >= 0; --r) {                       // descending: the lowest id is taken last
        if (r < R && q[r].z == RAFT_LEADER) {
            l.r = r;
            l.term = q[r].x;
            ++l.n;
        }
    }
    return l;
}

// The group's newest leader, the one a linearizable read asks (raft_read.hip):
// of the replicas whose role is LEADER the one with the highest currentTerm,
// the lowest index among equals.  Not find_leader's rule: a deposed leader
// keeps its role until it hears of the new term, and at a lower index it would
// shadow its successor.
__device__ __forceinline__ Lead find_newest_leader(const DevParams& p, int64_t g) {
    int4 q[RAFT_MAX_R];
    load_roles(p, g, q);
    const int R = p.R;
    Lead l{-1, 0, 0};
#pragma unroll
    for (int r = RAFT_MAX_R - 1; r >= 0; --r) {                       // descending: of equal terms the lowest id is taken last
        if (r < R && q[r].z == RAFT_LEADER) {
            ++l.n;
            if (l.r < 0 || q[r].x >= l.term) {
                l.r = r;
                l.term = q[r].x;
            }
        }
    }
    return l;
}

// ---- the selection of a drain (raft_apply.hip) or an apply (raft_sm.hip) of
// groups [g0, ...): every replica of each group (replica < 0), or one replica
// index per group; selected replica j is replica sel_idx(s, j)
struct Sel {
    int64_t g0, N;                                   // first group; selected replicas
    int32_t replica;
};

template <int R>
__device__ __forceinline__ int64_t sel_idx(const Sel& s, int64_t j) {
    return s.replica < 0 ? s.g0 * R + j : (s.g0 + j) * R + s.replica;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Fn<R>::run(a...) for the engine's R (their kernels are templated on it)
template <template <int> class Fn, typename... A>
void by_R(int R, A&&... a) {
    switch (R) {
        case 1: Fn<1>::run(a...); break;
        case 2: Fn<2>::run(a...); break;
        case 3: Fn<3>::run(a...); break;
        case 4: Fn<4>::run(a...); break;
        case 5: Fn<5>::run(a...); break;
        case 6: Fn<6>::run(a...); break;
        case 7: Fn<7>::run(a...); break;
        case 8: Fn<8>::run(a...); break;
        default: break;
    }
}

// The batch handlers report one thing: reference accesses below the window
// (the run is then invalid, RAFT_EWINDOW).  Called in divergent control flow:
// a mask's bit for this lane is read with ib().
struct BatchCounters {
    uint32_t miss = 0;
    __device__ __forceinline__ void add(uint64_t m, int c) {
        if (c == RAFT_C_LOG_WINDOW_MISS) miss += ib(m) ? 1u : 0u;
    }
};
}  // namespace

struct raft_engine {
    raft_params p;
    DevParams dp;
    int device;
    hipStream_t stream;
    void* base;
    size_t bytes;
    uint64_t t;
    int K;                      // steps per launch
    int nwaves;                 // chunks: ceil(G / (64 / R)), one wave's groups (and log block) each
    int nblocks;                // step-kernel workgroups of the one-chunk-per-wave schedule: ceil(nwaves / STEP_WAVES)
    int ncu;                    // compute units of the device
    // the launch schedule (raft_params.schedule, schedule_workgroups; step_kernel)
    int schedule, sched_wg;
    bool part_only;             // the workload's kernel is partitions-only (auto_subranges)
    raft_kernel_info last;      // the last step launch (raft_engine_kernel_info)
    static constexpr int OCC_SLOTS = 4;
    const void* occ_kern[OCC_SLOTS];   // workgroups per CU of occ_kern at occ_lds bytes of LDS (cached)
    size_t occ_lds[OCC_SLOTS];
    int occ_wg[OCC_SLOTS];
    uint32_t occ_next;
    uint32_t* partials;         // [K][NCW][nblocks] packed per-workgroup counter partials (buffer 0)
    uint32_t* partials2;        // buffer 1: launches alternate between the two when nsub > 1
    uint32_t* hpart;            // [K][NCW][workgroups] partials of a launch run as epochs (grow-only,
    size_t hpart_bytes;         // raft_engine_step_async)
    // launch sub-ranges (raft_engine_step_async): the step workgroups split
    // into nsub contiguous ranges, each launched on its own stream, so one
    // range's last waves overlap another's next launch instead of leaving
    // the chip part-empty at every launch boundary
    int nsub;
    int sub_b0[RAFT_MAX_SUBRANGES + 1];       // workgroup boundaries
    hipStream_t sub_stream[RAFT_MAX_SUBRANGES];
    hipEvent_t ev_fork, ev_sub_done[RAFT_MAX_SUBRANGES], ev_red_done[2];
    hipEvent_t ev_wait;         // raft_engine_wait_stream
    uint64_t launches_issued;   // step launches (all sub-ranges) so far: the partials buffer parity
    bool fork_needed;           // the engine stream holds work the sub-range streams have not waited for
    // batch path staging, grow-only: device scratch (keys, sort), device
    // copies of host batches, pinned host staging, pinned status flags
    char* bst;
    size_t bst_bytes;
    bool bst_dirty;             // the bucketed path's device status words may be nonzero (a batch failed mid-way)
    char* bio;
    size_t bio_bytes;
    char* hst;
    size_t hst_bytes;
    unsigned int* bflags_host;
    int batch_path;             // RAFT_BATCH_PATH_* (raft_engine_set_batch_path)
    char* aux;                  // device staging of the state / log / digest accessors, grow-only
    size_t aux_bytes;
    // committed-entry delivery (raft_apply.hip): lastApplied per replica [G * R], an allocation of its own
    // (never part of the state export or the digest), and the drain's grow-only staging: counts, offsets
    // and scan scratch (apl), the device copy of a host drain's records (apo)
    int32_t* applied;
    size_t applied_bytes;
    char* apl;
    size_t apl_bytes;
    char* apo;
    size_t apo_bytes;
    hipEvent_t ev_drain[5];     // pass boundaries of the last drain while drain_timing (scripts/drain_probe.py)
    bool drain_timing, drain_expanded;
    // the client path (raft_client.hip), grow-only: device scratch (keys, sort, status words) and the device
    // copies of a host call's arrays; host calls stage through hst like the batches
    char* cli;
    size_t cli_bytes;
    char* cio;
    size_t cio_bytes;
    // the replicated state machine (raft_sm.hip), opt-in: nullptr until raft_engine_sm_configure.  One
    // allocation: a 4-KB header (the totals of an apply, striped), the heads [G * R] of 16 bytes (applied, lost,
    // hash), the registers [G * R][sm_slots] uint32.  Not staging: trim_staging keeps it
    char* sm;
    size_t sm_bytes;
    int sm_slots;
    hipEvent_t ev_sm[2];        // around the last apply kernel while sm_timing (scripts/sm_probe.py)
    bool sm_timing;
    // raft_engine_sm_set_noop: while sm_noop_on an apply writes no register for an entry whose cmd is sm_noop_cmd.
    // The engine's, not the machine's: off at create, and reset / sm_configure / sm_write leave it alone
    bool sm_noop_on;
    uint32_t sm_noop_cmd;
    // the leader watch (raft_watch.hip): what it last reported per group [G] (leader, term), an allocation of
    // its own like lastApplied's; nullptr until the first call that needs it.  Not staging: trim_staging keeps it
    int2* watch;
    size_t watch_bytes;
    int64_t* counters_dev;      // [K][STRIDE] scratch
    unsigned long long* accum;  // [K * NC] counter accumulators: sum + chunks done << 48 (zero between launches)
    // step-kernel event timing
    bool cache_valid;           // log-tail cache (F_T1, F_T2, F_C1) matches state + logs: the step kernel and the
                                // handler batches keep it; write_state / write_log make it stale
    bool iso_written;           // write_state stored a nonzero isolation word (step_fn: NET_ISO kernels)
    bool timing;
    std::vector<hipEvent_t> ev;  // pool, pairs (one per sub-range launch)
    size_t ev_used;
    int64_t timed_launches;     // K-step launches of the whole grid timed since the last kernel_time()
};

namespace {
// ---- argument checks of the entry points: each sets raft_last_error()
// groups [g0, g0 + n) of an engine
inline int check_groups(raft_engine* e, int64_t g0, int64_t n) {
    if (!e) return raft_internal_fail(RAFT_EINVAL, "null engine");
    if (g0 < 0 || n < 0 || g0 + n > e->p.G) return raft_internal_fail(RAFT_ERANGE, "group range outside the engine");
    return RAFT_OK;
}
// a batch of n messages; any_null: one of its buffers is null (an error only when n > 0)
inline int check_args(raft_engine* e, int64_t n, bool any_null) {
    if (!e) return raft_internal_fail(RAFT_EINVAL, "null engine");
    if (n < 0) return raft_internal_fail(RAFT_EINVAL, "negative batch");
    if (n > 0x7FFFFFFF) return raft_internal_fail(RAFT_EINVAL, "batch larger than 2^31 - 1 messages");
    if (n > 0 && any_null) return raft_internal_fail(RAFT_EINVAL, "null buffer");
    return RAFT_OK;
}
// an engine whose state machine is configured
inline int check_sm(raft_engine* e) {
    if (!e) return raft_internal_fail(RAFT_EINVAL, "null engine");
    if (!e->sm)
        return raft_internal_fail(RAFT_EINVAL, "the state machine is not configured (raft_engine_sm_configure first)");
    return RAFT_OK;
}

// ---- a host call's arrays: copied into the engine's page-locked staging
// (hst), moved with one DMA to their device copies (cio); the records come
// back the same way.  Layout of both: up to 3 inputs, 256-byte aligned each,
// then the output.
struct Staged {
    size_t off[3];
    size_t out_off, out_bytes;
};
inline int stage_in(raft_engine* e, const void* const* src, const size_t* bytes, int k, size_t out_bytes, Staged& s) {
    size_t at = 0;
    for (int i = 0; i < k; ++i) {
        s.off[i] = at;
        at += al256(bytes[i]);
    }
    s.out_off = at;
    s.out_bytes = out_bytes;
    if (int rc = raft_internal_grow_dev(e, &e->cio, &e->cio_bytes, at + al256(out_bytes))) return rc;
    if (int rc = raft_internal_grow_host(e, &e->hst, &e->hst_bytes, at + al256(out_bytes))) return rc;
    for (int i = 0; i < k; ++i) std::memcpy(e->hst + s.off[i], src[i], bytes[i]);
    HIP_TRY(hipMemcpyAsync(e->cio, e->hst, at, hipMemcpyHostToDevice, e->stream));
    return RAFT_OK;
}
// the output's way back in its two halves -- the DMA into hst, and after a
// stream synchronize the copy to the caller -- for a call that decides in
// between whether the caller's memory is written (raft_engine_sm_get)
inline int stage_out_dma(raft_engine* e, const Staged& s) {
    HIP_TRY(hipMemcpyAsync(e->hst + s.out_off, e->cio + s.out_off, s.out_bytes, hipMemcpyDeviceToHost, e->stream));
    return RAFT_OK;
}
inline void stage_out_copy(raft_engine* e, const Staged& s, void* dst) { std::memcpy(dst, e->hst + s.out_off, s.out_bytes); }
inline int stage_out(raft_engine* e, const Staged& s, void* dst) {
    if (int rc = stage_out_dma(e, s)) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream));
    stage_out_copy(e, s, dst);
    return RAFT_OK;
}

// ---- the status words or totals a call's kernels leave on the device:
// STRIPES lines of LINE words of T, words 0 .. WORDS - 1 of a line in use.
// zero() clears them on the engine stream before the kernels; fetch() copies
// them back, waits for the stream and folds the stripes word by word into w[]
// (a sum, or an OR).  Why stripes: when most waves of a large call have
// something to report, one atomic each on a single word serialises them
// ("Measured", has the figure); a wave uses stripe (its index
// mod STRIPES) instead.  One stripe is the plain case: it lands in the engine's
// page-locked words (below the step kernel's, word 8), the striped ones in a
// local array.
template <typename T, int STRIPES, int LINE, int WORDS, bool SUM>
struct DevWords {
    static constexpr size_t BYTES = (size_t)STRIPES * LINE * sizeof(T);
    static_assert(WORDS <= LINE && (STRIPES > 1 || BYTES <= 8 * sizeof(unsigned int)), "one stripe fits bflags_host");
    T* dev;
    T w[WORDS];
    int zero(raft_engine* e, void* at) {
        dev = (T*)at;
        HIP_TRY(hipMemsetAsync(dev, 0, BYTES, e->stream));
        return RAFT_OK;
    }
    int fetch(raft_engine* e) {
        T local[STRIPES > 1 ? STRIPES * LINE : 1];
        T* h = STRIPES > 1 ? local : (T*)e->bflags_host;
        HIP_TRY(hipMemcpyAsync(h, dev, BYTES, hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        for (int i = 0; i < WORDS; ++i) {
            w[i] = 0;
            for (int k = 0; k < STRIPES; ++k) w[i] = SUM ? w[i] + h[k * LINE + i] : w[i] | h[k * LINE + i];
        }
        return RAFT_OK;
    }
};
// the totals of a state-machine apply (the header of raft_engine::sm) and of a restart: 64 lines of 64 bytes,
// 64-bit sums.  Their kernels index it with these.
constexpr int HDR_LINE = 8, HDR_STRIPES = 64;
using Totals = DevWords<unsigned long long, HDR_STRIPES, HDR_LINE, 3, true>;

// the machine's allocation (raft_engine::sm, raft_sm.hip): the totals header, the heads [G * R] (int4: applied,
// lost, hash lo, hash hi), the registers [G * R][sm_slots]; raft_fault.hip zeroes a restarted replica's
inline int4* sm_heads_of(raft_engine* e) { return (int4*)(e->sm + Totals::BYTES); }
inline uint32_t* sm_regs_of(raft_engine* e) { return (uint32_t*)(e->sm + Totals::BYTES + al256((size_t)e->dp.GR * 16)); }
inline int log2_slots(const raft_engine* e) {
    int l = 0;
    while ((1 << l) < e->sm_slots) ++l;
    return l;
}
}  // namespace
