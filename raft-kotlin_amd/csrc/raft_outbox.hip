// raft_outbox.hip — the proposal outbox (include/raft_engine.h
// raft_engine_outbox_configure, raft_outbox_submit*, raft_engine_outbox_pump*,
// raft_engine_outbox_read / write): a queue in HBM that holds proposals until
// they are committed, re-proposes exactly the ones no replica holds any more
// and hands completions out as a stream.  Raft thesis §6.3's "the client
// retries", made safe against duplicates without sessions; the reference has no
// counterpart.
//
// A side path between two step launches with kernels of its own; the step
// kernel, the canonical state and the digest do not know about it.  The queue
// is an array of 48-byte records (raft_outbox_entry as it is exported: three
// 16-byte quads) in one of two halves; a pump writes the survivors into the
// other half.
//
// Where it lives.  The engine object and raft_engine.hip belong to the step
// kernel's sources (build.py kernel_source_id) and stay as they are, so the
// outbox owns no engine member.  It shares the allocation of the engine's other
// per-consumer array that is kept apart from the state, the leader watch's
// (raft_engine::watch, raft_watch.hip): [seen pairs of G groups][a 256-byte
// outbox header][half 0][half 1].  That allocation is already freed by
// raft_engine_destroy, counted by raft_engine_device_bytes, kept by
// raft_engine_trim_staging and reset through raft_internal_watch_reset, which
// is all an outbox needs of the engine.  The header (capacity, length,
// expire_steps, the current half) is the outbox's only state: every call reads
// it at its start and stores it back when it changed, 40 bytes each way.  An
// outbox is configured iff the allocation is larger than the seen pairs.  The
// scratch of a pump is the drain's staging (apl), its host-form records go
// through apo and its gathered retries through cio, all grow-only staging that
// trim_staging frees.
//
// A pump, on the engine stream:
//   1. verdict   eight lanes per record, lane r for replica r, through the
//                resolve's own per-ticket routine (raft_ticket.h); the record's
//                lane 0 stores a one-byte verdict, each wave adds its counts to
//                its stripe of the totals, each workgroup stores the (done,
//                retry) count of its 32 records
//      -- the one read-back inside a pump: the totals.  Nothing done within
//         max_done and nothing to retry: the queue stays where it is --
//   2. scan      exclusive scan of the workgroups' counts (rocprim): n / 32
//                items.  Every order comes from it, never from an atomic.
//   3. split     one thread per record, one pass: ballots and a block scan
//                give its rank among the done and the retried records before
//                it; a done record within max_done goes to done[], every other
//                record to the other half at (its position - the done records
//                written before it), a retried one also to the gathered
//                (group, cmd, position) arrays; the COMMITTED ages are counted
//                in an LDS histogram per workgroup, then in striped words
//   4. propose   raft_propose_batch_dev's device path over the gathered arrays
//                (raft_internal_propose_enqueue): the propose's semantics by
//                construction.  Skipped when nothing retries.
//   5. scatter   one thread per retried record: its new ticket into the
//                survivor, tries + 1, the outcome counts per wave
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstddef>
#include <string>

#include "raft_ledger.h"
#include "raft_ticket.h"

using namespace raft;

namespace {

static_assert(sizeof(raft_outbox_entry) == 48 && sizeof(raft_outbox_done) == 32 && sizeof(raft_outbox_info) == 45 * 8,
              "record layouts of the C-ABI");

constexpr size_t REC = sizeof(raft_outbox_entry);
constexpr int TILE_RECS = BLOCK / RAFT_MAX_R;                           // records per verdict workgroup: 32

// verdicts, one byte per record
enum : uint8_t { V_PENDING = 0, V_ORPHANED = 1, V_UNKNOWN = 2, V_RETRY = 3, V_COMMITTED = 4, V_EXPIRED = 5, V_KINDS = 6 };
// the totals of a pump, striped as a restart's (64 lines of 128 bytes): the verdict counts by kind, then the
// outcomes of the re-proposal
enum { T_ACCEPTED = V_KINDS, T_GHOSTED, T_NO_LEADER, T_LOG_FULL, T_WORDS };
constexpr int TOT_LINE = 16;
using Tot = DevWords<unsigned long long, HDR_STRIPES, TOT_LINE, T_WORDS, true>;
constexpr int HIST_STRIPES = 16;
using Hist = DevWords<unsigned long long, HIST_STRIPES, 32, 32, true>;
using Flag = DevWords<unsigned int, 1, 4, 1, false>;                    // a submit's "group outside the engine"
// the head of a call's scratch (apl): totals, histogram, flag; then a pump's verdicts, counts, offsets and scan scratch
constexpr size_t OBS_TOT = 0, OBS_HIST = Tot::BYTES, OBS_FLAG = OBS_HIST + Hist::BYTES, OBS_HEAD = OBS_FLAG + 256;

// the outbox's header in HBM, behind the watch's seen pairs, and its copy during a call
constexpr size_t OB_HDR = 256;
constexpr int64_t OB_MAGIC = 0x786f6274756f;                            // "outbox"
struct Ob {
    int64_t magic, cap, len, expire, half;                              // (the header's words)
};
inline size_t seen_bytes(const raft_engine* e) { return al256((size_t)e->p.G * sizeof(int2)); }
inline bool configured(const raft_engine* e) { return e->watch && e->watch_bytes > seen_bytes(e); }
inline char* ob_hdr(raft_engine* e) { return (char*)e->watch + seen_bytes(e); }
inline int4* half_of(raft_engine* e, int64_t h) {
    return (int4*)(ob_hdr(e) + OB_HDR + (size_t)h * ((e->watch_bytes - seen_bytes(e) - OB_HDR) / 2));
}
int ob_load(raft_engine* e, Ob& ob) {
    if (int rc = rows_out(e, ob_hdr(e), sizeof(Ob), &ob)) return rc;
    if (ob.magic != OB_MAGIC || ob.cap < 1 || ob.len < 0 || ob.len > ob.cap || (ob.half & ~(int64_t)1))
        return raft_internal_fail(RAFT_EDEVICE, "the outbox's header is damaged");
    return RAFT_OK;
}
int ob_store(raft_engine* e, const Ob& ob) { return rows_in(e, ob_hdr(e), &ob, sizeof(Ob)); }

__device__ __forceinline__ int64_t i64_of(int32_t lo, int32_t hi) {
    return (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint64_t)(uint32_t)lo);
}
__device__ __forceinline__ int32_t clip32(int64_t x) {
    return (int32_t)min((int64_t)INT_MAX, max((int64_t)INT_MIN, x));
}

// records [len, len + n) of the queue: (tag, born | group, cmd, -1, -1 | 0, NEW, 0, 0)
__global__ __launch_bounds__(BLOCK) void outbox_submit_kernel(int4* __restrict__ q, int64_t len,
                                                              const int64_t* __restrict__ group,
                                                              const uint32_t* __restrict__ cmd,
                                                              const int64_t* __restrict__ tag, int64_t n, int64_t born,
                                                              int64_t G, unsigned int* flag) {
    const int64_t j = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n) return;                                                 // len + n <= capacity (the host checked)
    const int64_t g = group[j], t = tag[j];
    if (g < 0 || g >= G) *(volatile unsigned int*)flag = 1u;            // (idempotent plain store; the tail is not advanced)
    int4* r = q + 3 * (len + j);
    r[0] = make_int4((int32_t)(uint32_t)(uint64_t)t, (int32_t)(uint32_t)((uint64_t)t >> 32),
                     (int32_t)(uint32_t)(uint64_t)born, (int32_t)(uint32_t)((uint64_t)born >> 32));
    r[1] = make_int4((int32_t)g, (int32_t)cmd[j], -1, -1);
    r[2] = make_int4(0, RAFT_OUTBOX_NEW, 0, 0);
}

// pass 1.  Eight lanes per record; every lane of a workgroup stays to the end
// (the shuffles and the barrier), lanes past the last record read the last one
// and count nothing.
__global__ __launch_bounds__(BLOCK) void outbox_verdict_kernel(DevParams p, const int4* __restrict__ q, int64_t n,
                                                               int64_t now, int32_t expire,
                                                               uint8_t* __restrict__ verdict,
                                                               unsigned long long* __restrict__ tcnt,
                                                               unsigned long long* tot) {
    __shared__ unsigned long long wc[WAVES_PER_BLOCK];
    const int64_t tid = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const int r = (int)(tid & 7);
    const bool live = (tid >> 3) < n;
    const int64_t m = live ? tid >> 3 : n - 1;
    const int4 q0 = q[3 * m], q1 = q[3 * m + 1], q2 = q[3 * m + 2];
    const int64_t g = q1.x;
    const int4 tk = make_int4(q1.z, q1.w, q2.x, q2.y);                  // (replica, index, term, status)
    const bool stored = tk.w != RAFT_PROPOSE_NO_LEADER && tk.w != RAFT_PROPOSE_LOG_FULL && tk.w != RAFT_OUTBOX_NEW;
    const uint32_t v = ticket_sum(ticket_lane(p, g, tk, (uint32_t)q1.y, r, stored));
    const TicketVerdict o = ticket_verdict(p, g, tk, stored, v);
    const int64_t age = now - i64_of(q0.z, q0.w);
    uint8_t code;
    if (o.status == RAFT_TICKET_COMMITTED) code = V_COMMITTED;
    else if (expire > 0 && age >= expire) code = V_EXPIRED;
    else if (o.status == RAFT_TICKET_UNKNOWN || o.status == RAFT_TICKET_INVALID) code = V_UNKNOWN;  // (INVALID: outbox_write refuses it)
    else if (o.status == RAFT_TICKET_PENDING) code = V_PENDING;
    else if (o.status == RAFT_TICKET_LOST && o.holders >= 1) code = V_ORPHANED;
    else code = V_RETRY;                                                // LOST on no replica, or NONE
    const bool lead = live && r == 0;
    if (lead) verdict[m] = code;
    uint32_t cnt[V_KINDS];
#pragma unroll
    for (int k = 0; k < V_KINDS; ++k) cnt[k] = (uint32_t)__popcll(__ballot(lead && code == k));
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) {
        unsigned long long* line = stripe_of(tot, wave_index(), TOT_LINE);
#pragma unroll
        for (int k = 0; k < V_KINDS; ++k) tally(line, k, cnt[k]);
        wc[wv] = ((unsigned long long)(cnt[V_COMMITTED] + cnt[V_EXPIRED]) << 32) | cnt[V_RETRY];
    }
    __syncthreads();
    if (threadIdx.x == 0) {                                             // (done, retry) of this workgroup's 32 records
        unsigned long long s = 0;
#pragma unroll
        for (int w = 0; w < WAVES_PER_BLOCK; ++w) s += wc[w];
        tcnt[blockIdx.x] = s;
    }
}

// pass 3.  Workgroup b owns records [256 b, 256 b + 256): the counts of eight
// verdict workgroups, so its carry is off[8 b] = (done, retry) before it.
__global__ __launch_bounds__(BLOCK) void outbox_split_kernel(const int4* __restrict__ q, int4* __restrict__ q_out,
                                                             const uint8_t* __restrict__ verdict,
                                                             const unsigned long long* __restrict__ off, int64_t n,
                                                             int64_t max_done, int64_t now, int4* __restrict__ done,
                                                             int64_t* __restrict__ rg, uint32_t* __restrict__ rc,
                                                             uint32_t* __restrict__ rpos, unsigned long long* hist) {
    __shared__ uint32_t wd[WAVES_PER_BLOCK], wr[WAVES_PER_BLOCK], lh[32];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t m = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const bool live = m < n;
    const uint8_t code = live ? verdict[m] : (uint8_t)V_PENDING;
    const bool is_done = code >= V_COMMITTED, is_retry = code == V_RETRY;
    const uint64_t bd = __ballot(is_done), br = __ballot(is_retry), below = (1ull << lane) - 1ull;
    if (threadIdx.x < 32) lh[threadIdx.x] = 0u;
    if (lane == 0) {
        wd[wv] = (uint32_t)__popcll(bd);
        wr[wv] = (uint32_t)__popcll(br);
    }
    __syncthreads();
    const unsigned long long carry = off[(int64_t)blockIdx.x * (BLOCK / TILE_RECS)];
    int64_t d_before = (int64_t)(carry >> 32) + __popcll(bd & below);
    int64_t r_before = (int64_t)(carry & 0xFFFFFFFFull) + __popcll(br & below);
    for (int w = 0; w < wv; ++w) {
        d_before += wd[w];
        r_before += wr[w];
    }
    if (live) {
        const int4 q0 = q[3 * m], q1 = q[3 * m + 1], q2 = q[3 * m + 2];
        if (is_done && d_before < max_done) {                           // inside done[]: d_before < max_done
            const int32_t age = clip32(now - i64_of(q0.z, q0.w));
            done[2 * d_before] = make_int4(q0.x, q0.y, q1.x, code == V_COMMITTED ? RAFT_OUTBOX_COMMITTED : RAFT_OUTBOX_EXPIRED);
            done[2 * d_before + 1] = make_int4(q1.w, q2.x, q2.z, age);  // index, term, tries, age
            if (code == V_COMMITTED)
                atomicAdd(&lh[min(31, 63 - __builtin_clzll((unsigned long long)max(age, 0) + 1ull))], 1u);
        } else {                                                        // a survivor: 0 <= pos <= m < capacity
            const int64_t pos = m - min(d_before, max_done);
            q_out[3 * pos] = q0;
            q_out[3 * pos + 1] = q1;
            q_out[3 * pos + 2] = q2;
            if (is_retry) {                                             // r_before < the retry total: inside the arrays
                rg[r_before] = q1.x;
                rc[r_before] = (uint32_t)q1.y;
                rpos[r_before] = (uint32_t)pos;
            }
        }
    }
    __syncthreads();
    if (threadIdx.x < 32 && lh[threadIdx.x])
        atomicAdd(hist + (blockIdx.x & (HIST_STRIPES - 1)) * 32 + threadIdx.x, (unsigned long long)lh[threadIdx.x]);
}

// pass 5.  Retried record j (queue order) is the survivor at rpos[j].
__global__ __launch_bounds__(BLOCK) void outbox_scatter_kernel(int4* __restrict__ q_out, const uint32_t* __restrict__ rpos,
                                                               const int4* __restrict__ ticket, int64_t n,
                                                               unsigned long long* tot) {
    const int64_t j = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const bool live = j < n;
    int32_t st = -1;
    if (live) {
        const int4 tk = ticket[j];                                      // (replica, index, term, status)
        int4* r = q_out + 3 * (int64_t)rpos[j];
        const int4 q1 = r[1], q2 = r[2];
        r[1] = make_int4(q1.x, q1.y, tk.x, tk.y);
        r[2] = make_int4(tk.z, tk.w, q2.z + 1, 0);
        st = tk.w;
    }
    const uint64_t b[4] = {__ballot(st == RAFT_PROPOSE_ACCEPTED), __ballot(st == RAFT_PROPOSE_GHOSTED),
                           __ballot(st == RAFT_PROPOSE_NO_LEADER), __ballot(st == RAFT_PROPOSE_LOG_FULL)};
    if ((threadIdx.x & 63) == 0) {
        unsigned long long* line = stripe_of(tot, wave_index(), TOT_LINE);
#pragma unroll
        for (int k = 0; k < 4; ++k) tally_ballot(line, T_ACCEPTED + k, b[k]);
    }
}

int check_outbox(raft_engine* e) {
    if (!e) return raft_internal_fail(RAFT_EINVAL, "null engine");
    if (!configured(e))
        return raft_internal_fail(RAFT_EINVAL, "the outbox is not configured (raft_engine_outbox_configure first)");
    return RAFT_OK;
}

int submit(raft_engine* e, const int64_t* group, const uint32_t* cmd, const int64_t* tag, int64_t n, bool on_host) {
    if (int rc = check_outbox(e)) return rc;
    if (n < 0) return raft_internal_fail(RAFT_EINVAL, "negative batch");
    if (n == 0) return RAFT_OK;
    if (!group || !cmd || !tag) return raft_internal_fail(RAFT_EINVAL, "null buffer");
    Ob ob;
    if (int rc = ob_load(e, ob)) return rc;
    if (n > ob.cap - ob.len)
        return raft_internal_fail(RAFT_EFULL, "the outbox has room for " + std::to_string(ob.cap - ob.len) +
                                                  " records, the batch has " + std::to_string(n) + ": nothing was enqueued");
    HIP_TRY(hipSetDevice(e->device));
    if (on_host) {
        for (int64_t j = 0; j < n; ++j)
            if (group[j] < 0 || group[j] >= e->p.G)
                return raft_internal_fail(RAFT_ERANGE, "a record's group is outside the engine: nothing was enqueued");
        const void* src[3] = {group, cmd, tag};
        const size_t bytes[3] = {(size_t)n * 8, (size_t)n * 4, (size_t)n * 8};
        Staged s;
        if (int rc = stage_in(e, src, bytes, 3, 0, s)) return rc;
        group = (const int64_t*)(e->cio + s.off[0]);
        cmd = (const uint32_t*)(e->cio + s.off[1]);
        tag = (const int64_t*)(e->cio + s.off[2]);
    }
    if (int rc = raft_internal_grow_dev(e, &e->apl, &e->apl_bytes, OBS_HEAD)) return rc;
    Flag f;
    if (int rc = f.zero(e, e->apl + OBS_FLAG)) return rc;
    outbox_submit_kernel<<<grid_of(n), BLOCK, 0, e->stream>>>(
        half_of(e, ob.half), ob.len, group, cmd, tag, n, (int64_t)e->t, e->p.G, f.dev);
    HIP_TRY(hipGetLastError());
    if (int rc = f.fetch(e)) return rc;
    if (f.w[0])                                                        // (the tail stays: what was written is not in the queue)
        return raft_internal_fail(RAFT_ERANGE, "a record's group is outside the engine: nothing was enqueued");
    ob.len += n;
    return ob_store(e, ob);
}

int pump(raft_engine* e, raft_outbox_done* done, int64_t max_done, int64_t* n_done, raft_outbox_info* info,
         bool on_host) {
    if (int rc = check_outbox(e)) return rc;
    if (!n_done || !info) return raft_internal_fail(RAFT_EINVAL, "null n_done or info");
    *n_done = 0;
    *info = raft_outbox_info{};
    if (int rc = check_records(done, max_done, on_host, 16, "max_done")) return rc;
    Ob ob;
    if (int rc = ob_load(e, ob)) return rc;
    const int64_t n = ob.len;
    if (n == 0) return RAFT_OK;
    e->fork_needed = true;                           // later step launches wait for these reads of the state and logs
    const size_t ntile = (size_t)((n + TILE_RECS - 1) / TILE_RECS);
    ScanScratch<unsigned long long> sc;              // the packed (done, retry) counts; the verdicts end the head
    if (int rc = sc.init(e, &e->apl, &e->apl_bytes, OBS_HEAD + al256((size_t)n), ntile)) return rc;
    uint8_t* verdict = (uint8_t*)(sc.head + OBS_HEAD);
    Tot tot;
    Hist hist;
    if (int rc = tot.zero(e, sc.head + OBS_TOT)) return rc;
    if (int rc = hist.zero(e, sc.head + OBS_HIST)) return rc;
    const int4* q = half_of(e, ob.half);
    const int64_t now = (int64_t)e->t;
    outbox_verdict_kernel<<<(unsigned)ntile, BLOCK, 0, e->stream>>>(e->dp, q, n, now, (int32_t)ob.expire, verdict, sc.cnt, tot.dev);
    HIP_TRY(hipGetLastError());
    if (int rc = tot.fetch(e)) return rc;            // the read-back inside a pump: what is done, what retries
    const int64_t n_fin = (int64_t)(tot.w[V_COMMITTED] + tot.w[V_EXPIRED]), n_retry = (int64_t)tot.w[V_RETRY];
    const int64_t emitted = std::min(n_fin, max_done);
    info->queued = n;
    info->deferred = n_fin - emitted;
    info->pending = (int64_t)tot.w[V_PENDING];
    info->orphaned = (int64_t)tot.w[V_ORPHANED];
    info->unknown = (int64_t)tot.w[V_UNKNOWN];
    info->retried = n_retry;
    info->left = n - emitted;
    int prc = RAFT_OK;
    if (emitted > 0 || n_retry > 0) {
        Records rec;                                                   // (nothing emitted: nothing staged or copied back)
        if (int rc = rec.begin(e, done, (size_t)emitted * sizeof(raft_outbox_done), on_host)) return rc;
        // the gathered retries, in the client path's staging: groups, commands, positions, the new tickets
        const size_t g_b = al256((size_t)n_retry * 8), u_b = al256((size_t)n_retry * 4), t_b = al256((size_t)n_retry * 16);
        if (n_retry > 0)
            if (int rc = raft_internal_grow_dev(e, &e->cio, &e->cio_bytes, g_b + 2 * u_b + t_b)) return rc;
        char* const rb = n_retry > 0 ? e->cio : nullptr;               // (nothing retries: the split stores none)
        int64_t* rg = (int64_t*)rb;
        uint32_t* rc_ = (uint32_t*)(rb + g_b);
        uint32_t* rpos = (uint32_t*)(rb + g_b + u_b);
        raft_ticket* rtk = (raft_ticket*)(rb + g_b + 2 * u_b);
        if (int rc = sc.run(e)) return rc;
        int4* q_out = half_of(e, ob.half ^ 1);
        outbox_split_kernel<<<grid_of(n), BLOCK, 0, e->stream>>>(
            q, q_out, verdict, sc.off, n, max_done, now, (int4*)rec.dev, rg, rc_, rpos, hist.dev);
        HIP_TRY(hipGetLastError());
        if (n_retry > 0) {
            if (int rc = raft_internal_propose_enqueue(e, rg, rc_, rtk, (int)n_retry)) return rc;
            outbox_scatter_kernel<<<grid_of(n_retry), BLOCK, 0, e->stream>>>(
                q_out, rpos, (const int4*)rtk, n_retry, tot.dev);
            HIP_TRY(hipGetLastError());
        }
        // from here on the other half is the queue, whatever the propose reports
        ob.half ^= 1;
        ob.len = n - emitted;
        HIP_TRY(hipMemcpyAsync(ob_hdr(e), &ob, sizeof(Ob), hipMemcpyHostToDevice, e->stream));   // (waited for below)
        if (int rc = rec.finish(e)) return rc;
        if (n_retry > 0) {
            prc = raft_internal_propose_finish(e);
            if (prc != RAFT_OK && prc != RAFT_EWINDOW) return prc;
        }
        if (int rc = tot.fetch(e)) return rc;
        if (int rc = hist.fetch(e)) return rc;
        info->accepted = (int64_t)tot.w[T_ACCEPTED];
        info->ghosted = (int64_t)tot.w[T_GHOSTED];
        info->no_leader = (int64_t)tot.w[T_NO_LEADER];
        info->log_full = (int64_t)tot.w[T_LOG_FULL];
        for (int k = 0; k < 32; ++k) {
            info->age_hist[k] = (int64_t)hist.w[k];
            info->committed += (int64_t)hist.w[k];
        }
        info->expired = emitted - info->committed;
    }
    *n_done = emitted;
    if (info->unknown > 0 && prc == RAFT_OK)
        return raft_internal_fail(RAFT_EWINDOW, std::to_string(info->unknown) +
                                                    " records' tickets name a slot below a replica's log_window (kept)");
    return prc;
}

}  // namespace

// raft_watch.hip, raft_internal_watch_reset (raft_engine_reset): a configured outbox is empty again
int raft_internal_outbox_reset(raft_engine* e) {
    if (!configured(e)) return RAFT_OK;
    HIP_TRY(hipMemsetAsync(ob_hdr(e) + offsetof(Ob, len), 0, sizeof(int64_t), e->stream));
    return RAFT_OK;
}

extern "C" {

int raft_engine_outbox_configure(raft_engine* e, int64_t capacity, int32_t expire_steps) {
    if (!e) return raft_internal_fail(RAFT_EINVAL, "null engine");
    if (capacity < 1 || capacity > 0x7FFFFFFF || expire_steps < 0)
        return raft_internal_fail(RAFT_EINVAL, "the outbox needs 1 <= capacity < 2^31 and expire_steps >= 0");
    HIP_TRY(hipSetDevice(e->device));
    if (configured(e)) {
        Ob old;
        if (int rc = ob_load(e, old)) return rc;
        if (old.len > 0) return raft_internal_fail(RAFT_EINVAL, "the outbox is not empty: it cannot be configured again");
    }
    HIP_TRY(hipStreamSynchronize(e->stream));
    // a new allocation for the watch's seen pairs and the queue; the pairs move over, or start as "nothing reported"
    const size_t seen_b = seen_bytes(e), bytes = seen_b + OB_HDR + 2 * al256((size_t)capacity * REC);
    char* block = nullptr;
    if (hipMalloc((void**)&block, bytes) != hipSuccess) {
        (void)hipGetLastError();
        return raft_internal_fail(RAFT_ENOMEM, "the outbox's queue: " + std::to_string(bytes) + " bytes of device memory");
    }
    const bool had_watch = e->watch != nullptr;
    if (had_watch) {
        HIP_TRY(hipMemcpyAsync(block, e->watch, std::min(seen_b, e->watch_bytes), hipMemcpyDeviceToDevice, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        HIP_TRY(hipFree(e->watch));
    }
    e->watch = (int2*)block;
    e->watch_bytes = bytes;
    const Ob ob{OB_MAGIC, capacity, 0, expire_steps, 0};
    if (int rc = ob_store(e, ob)) return rc;
    if (!had_watch)
        if (int rc = raft_internal_watch_reset(e)) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream));
    return RAFT_OK;
}

int raft_outbox_submit(raft_engine* e, const int64_t* group, const uint32_t* cmd, const int64_t* tag, int64_t n) {
    return submit(e, group, cmd, tag, n, true);
}

int raft_outbox_submit_dev(raft_engine* e, const int64_t* group_dev, const uint32_t* cmd_dev, const int64_t* tag_dev,
                           int64_t n) {
    return submit(e, group_dev, cmd_dev, tag_dev, n, false);
}

int raft_engine_outbox_pump(raft_engine* e, raft_outbox_done* done_host, int64_t max_done, int64_t* n_done,
                            raft_outbox_info* info) {
    return pump(e, done_host, max_done, n_done, info, true);
}

int raft_engine_outbox_pump_dev(raft_engine* e, raft_outbox_done* done_dev, int64_t max_done, int64_t* n_done,
                                raft_outbox_info* info) {
    return pump(e, done_dev, max_done, n_done, info, false);
}

int raft_engine_outbox_read(raft_engine* e, raft_outbox_entry* out, int64_t room, int64_t* n) {
    if (int rc = check_outbox(e)) return rc;
    if (!n) return raft_internal_fail(RAFT_EINVAL, "null n");
    Ob ob;
    if (int rc = ob_load(e, ob)) return rc;
    *n = ob.len;
    if (!out && room == 0) return RAFT_OK;           // a peek: the queue's length
    if (!out || room < ob.len) return raft_internal_fail(RAFT_EINVAL, "the buffer has no room for the queue");
    if (ob.len == 0) return RAFT_OK;
    return rows_out(e, half_of(e, ob.half), (size_t)ob.len * REC, out);
}

int raft_engine_outbox_write(raft_engine* e, const raft_outbox_entry* in, int64_t n) {
    if (int rc = check_outbox(e)) return rc;
    if (n < 0 || (n > 0 && !in)) return raft_internal_fail(RAFT_EINVAL, "negative count or null buffer");
    Ob ob;
    if (int rc = ob_load(e, ob)) return rc;
    if (n > ob.cap) return raft_internal_fail(RAFT_EFULL, "more records than the outbox's capacity: nothing was stored");
    for (int64_t k = 0; k < n; ++k) {
        const raft_outbox_entry& r = in[k];
        if (r.group < 0 || r.group >= e->p.G)
            return raft_internal_fail(RAFT_ERANGE, "a record's group is outside the engine: nothing was stored");
        const bool known = r.status == RAFT_OUTBOX_NEW || (r.status >= RAFT_PROPOSE_ACCEPTED && r.status <= RAFT_PROPOSE_CURRENT);
        const bool stored = known && r.status != RAFT_OUTBOX_NEW && r.status != RAFT_PROPOSE_NO_LEADER &&
                            r.status != RAFT_PROPOSE_LOG_FULL;
        if (!known || r.tries < 0 || r.pad != 0 ||
            (stored && (r.replica < -1 || r.replica >= e->p.R || r.index < 0 || r.index >= e->p.log_cap)))
            return raft_internal_fail(RAFT_EINVAL, "a record's ticket (status, replica, index), tries or pad is outside "
                                                   "what a pump accepts: nothing was stored");
    }
    if (n > 0)
        if (int rc = rows_in(e, half_of(e, ob.half), in, (size_t)n * REC)) return rc;
    ob.len = n;
    return ob_store(e, ob);
}

}  // extern "C"
