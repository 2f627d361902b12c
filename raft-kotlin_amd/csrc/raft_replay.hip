// raft_replay.hip — WAL replay on the device (include/ext/raft_replay.h
// raft_wal_replay*): the inverse of raft_wal_poll.  A batch of raft_wal_records
// is applied to the replicas it names, in HBM, between two step launches: a
// replica gets its hard state and log back from its own disk after
// RAFT_RESTART_AMNESIA, or a second engine is kept in step with the first from
// raft_wal_poll_dev's buffer, without a host copy of a record.  The reference
// persists nothing and has no counterpart.
//
// Two kernels, one thread per record in both; a replica's run of records may
// span waves and workgroups, so no pass needs a fact from farther away than a
// record's neighbours (and, on a ring, the one record log_window places on).
//   validate   record m against records m - 1, m + 1 (and m + W on a ring) and
//              the target's lastIndex (quad 1), which only a TRUNCATE and an
//              ENTRY that follows no TRUNCATE and no ENTRY read.  Why local
//              checks are enough: the order rule makes a replica's records one
//              contiguous run; inside it each ENTRY is tied to its predecessor
//              (index + 1, or a TRUNCATE's keep, or the target's lastIndex), so
//              by induction the run's ENTRYs are consecutive indices below
//              log_cap, distinct slots of a flat row; on a ring two of them
//              share a slot only when they lie exactly W records apart, which
//              is the m + W check.  malformed, the per-kind totals and the run
//              heads go into a stripe, one atomic per wave and nonzero word
//              (DevWords, raft_engine_impl.h).  It writes nothing else.
//   (host)     reads the totals; any malformed record fails the call here,
//              before a word of engine state is written.
//   apply      an ENTRY stores its 8-byte slot into the replica's row
//              (install_kernel's row addressing).  The FIRST record of a run
//              (told from its predecessor) owns quad 0 (term and vote from a
//              HARDSTATE, role and flags), retryMs of quad 3, the replica's
//              session rows in spill and GX_S0.  The LAST record of a run (told
//              from its successor) owns quads 1 and 2: lastIndex, physLen, the
//              tail cache, electionMs, commitIndex, phaseMs.  The tail cache
//              comes from the records where the last one or two are ENTRYs,
//              else from log slots below what this batch writes (below a
//              TRUNCATE's keep or the lastIndex the first ENTRY stands on).  No
//              word has two writers and no atomic touches engine state.
//              Quad 3's other words are the primary session's column towards
//              this replica -- another replica's row -- and stay (restart_kernel's
//              rule): when this replica owned the slot, GX_S0 = -1 makes them dead.
// The volatile words are raft_engine_restart's with flags 0 (raft_fault.hip),
// the election timeout drawn from the same Philox word at the engine's step
// index.  The host form stages the records like a side path's batch (Staged).
#include <hip/hip_runtime.h>

#include <string>

#include "ext/raft_replay.h"
#include "raft_stream.h"

using namespace raft;

namespace {

static_assert(sizeof(raft_wal_record) == 24 && sizeof(raft_replay_info) == 64, "record layouts of the C-ABI");

// the totals of a replay, striped
enum { RW_MALFORMED = 0, RW_HS, RW_TR, RW_EN, RW_REPLICAS, RW_WORDS };
using ReplayTotals = DevWords<unsigned long long, HDR_STRIPES, HDR_LINE, RW_WORDS, true>;

// a record as three 8-byte words: (group, replica | kind << 16), (index, term), (cmd, aux)
struct Rec {
    int32_t g, r, kind, index, term;
    uint32_t cmd;
    int32_t aux;
};
__device__ __forceinline__ int32_t replica_of(uint2 w0) { return (int16_t)(w0.y & 0xFFFFu); }
__device__ __forceinline__ int32_t kind_of(uint2 w0) { return (int16_t)(w0.y >> 16); }
__device__ __forceinline__ Rec load_rec(const uint2* __restrict__ rec, int64_t m) {
    const uint2 a = rec[3 * m], b = rec[3 * m + 1], c = rec[3 * m + 2];
    return Rec{(int32_t)a.x, replica_of(a), kind_of(a), (int32_t)b.x, (int32_t)b.y, c.x, (int32_t)c.y};
}
__device__ __forceinline__ bool same_replica(uint2 w0, const Rec& x) {
    return (int32_t)w0.x == x.g && replica_of(w0) == x.r;
}

// the log row of replica r of group g (log_of with a compile-time R); g < G, r < R
template <int R>
__device__ __forceinline__ uint2* row_of(const DevParams& p, int32_t g, int32_t r) {
    constexpr int GPW = 64 / R;
    const int64_t w = g / GPW;
    return p.log + (w * 64 + ((g - w * GPW) * R + r)) * (int64_t)p.nslots;
}

// pass 1.  The rule of include/ext/raft_replay.h, record by record; nothing is written but the totals.
template <int R>
__global__ __launch_bounds__(BLOCK) void replay_validate_kernel(DevParams p, const uint2* __restrict__ rec, int64_t n,
                                                                unsigned long long* hdr) {
    const int64_t m = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    bool bad = false, head = false;
    int32_t kind = -1;
    if (m < n) {
        const Rec x = load_rec(rec, m);
        kind = x.kind;
        bool same = false;
        int32_t pk = -1, pindex = 0;
        if (m > 0) {
            const uint2 a = rec[3 * (m - 1)];
            const int32_t pg = (int32_t)a.x, pr = replica_of(a);
            pk = kind_of(a);
            same = pg == x.g && pr == x.r;
            bad = pg > x.g || (pg == x.g && pr > x.r);                  // the order of the runs
            if (same) pindex = (int32_t)rec[3 * (m - 1) + 1].x;
        }
        head = !same;
        bad |= x.g < 0 || x.g >= p.G || x.r < 0 || x.r >= R || kind < RAFT_WAL_HARDSTATE || kind > RAFT_WAL_ENTRY;
        if (!bad && same) bad = pk > kind || (pk == kind && kind != RAFT_WAL_ENTRY);   // HARDSTATE, TRUNCATE, ENTRY...
        if (!bad) {
            if (kind == RAFT_WAL_HARDSTATE) {
                bad = x.term < 0 || x.aux < -1 || x.aux > R;
            } else {
                const bool after_en = same && pk == RAFT_WAL_ENTRY, after_tr = same && pk == RAFT_WAL_TRUNCATE;
                if (kind == RAFT_WAL_TRUNCATE || !(after_en || after_tr)) {
                    // judged against the target now: in range, so the quad is inside the state
                    const int32_t last = max(0, min(quad(p, 1, (int64_t)x.g * R + x.r)->x, p.cap));
                    if (kind == RAFT_WAL_TRUNCATE) bad = x.index < 0 || x.index > last;
                    else bad = p.W != FLAT_W ? x.index < last : x.index != last;
                } else {
                    bad = x.index != (after_en ? (int64_t)pindex + 1 : (int64_t)pindex);
                }
                if (kind == RAFT_WAL_ENTRY) {
                    bad |= x.index < 0 || x.index >= p.cap;
                    if (p.W != FLAT_W && m + p.W < n) bad |= same_replica(rec[3 * (m + p.W)], x);   // one ring slot twice
                }
            }
        }
    }
    const unsigned long long b_bad = __ballot(bad), b_hd = __ballot(head);
    const unsigned long long b_hs = __ballot(kind == RAFT_WAL_HARDSTATE), b_tr = __ballot(kind == RAFT_WAL_TRUNCATE);
    const unsigned long long b_en = __ballot(kind == RAFT_WAL_ENTRY);
    if ((threadIdx.x & 63) == 0) {
        unsigned long long* line = stripe_of(hdr, wave_index());
        tally_ballot(line, RW_MALFORMED, b_bad);
        tally_ballot(line, RW_HS, b_hs);
        tally_ballot(line, RW_TR, b_tr);
        tally_ballot(line, RW_EN, b_en);
        tally_ballot(line, RW_REPLICAS, b_hd);
    }
}

// pass 2, only after a batch without a malformed record: every group, replica and slot below is inside the engine.
template <int R>
__global__ __launch_bounds__(BLOCK) void replay_apply_kernel(DevParams p, const uint2* __restrict__ rec, int64_t n,
                                                             uint32_t t, uint32_t flags) {
    const int64_t m = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (m >= n) return;
    const Rec x = load_rec(rec, m);
    const bool keepv = flags & RAFT_REPLAY_KEEP_VOLATILE;               // uniform
    bool first = true, last = true, after_en = false;
    int32_t pterm = 0;
    if (m > 0) {
        const uint2 a = rec[3 * (m - 1)];
        first = !same_replica(a, x);
        after_en = !first && kind_of(a) == RAFT_WAL_ENTRY;
        if (after_en) pterm = (int32_t)rec[3 * (m - 1) + 1].y;
    }
    if (m + 1 < n) last = !same_replica(rec[3 * (m + 1)], x);
    const int64_t idx = (int64_t)x.g * R + x.r;
    uint2* row = row_of<R>(p, x.g, x.r);
    if (x.kind == RAFT_WAL_ENTRY) row[(uint32_t)x.index & p.wmask] = make_uint2((uint32_t)x.term, x.cmd);
    if (first) {
        const bool hs = x.kind == RAFT_WAL_HARDSTATE;                  // a run's HARDSTATE is its first record
        if (hs || !keepv) {
            const int4 q0 = *quad(p, 0, idx);
            *quad(p, 0, idx) = make_int4(hs ? x.term : q0.x, hs ? x.aux : q0.y, keepv ? q0.z : RAFT_FOLLOWER,
                                         keepv ? q0.w : (int32_t)FL_ARMED);
        }
        if (!keepv) {
            p.st[fidx(p, RAFT_F_RETRY_MS, idx)] = 0;
            // rows next[r][*] / match[r][*]: spill[(g * R + d) * R + r] for every column d
            const int64_t base = (int64_t)x.g * R;
#pragma unroll
            for (int d = 0; d < R; ++d) {
                p.spill[(base + d) * R + x.r] = 0;
                p.spill[p.GR * R + (base + d) * R + x.r] = 0;
            }
            // at most one replica of a group owns the primary slot: one writer
            if (p.gx[GX_S0 * p.G + x.g] == x.r) p.gx[GX_S0 * p.G + x.g] = -1;
        }
    }
    if (last) {
        const int4 q1 = *quad(p, 1, idx), q2 = *quad(p, 2, idx);
        int32_t len = q1.x, phys = q1.y, t1 = q1.z, t2 = q2.y, c1 = q2.z;   // a HARDSTATE alone: the log stays
        if (x.kind == RAFT_WAL_ENTRY) {
            len = phys = x.index + 1;
            t1 = x.term;
            c1 = (int32_t)x.cmd;
            // the entry before: the record before, else a slot this batch does not write
            t2 = after_en ? pterm : x.index >= 1 ? (int32_t)row[(uint32_t)(x.index - 1) & p.wmask].x : 0;
        } else if (x.kind == RAFT_WAL_TRUNCATE) {                       // the run holds no ENTRY: slots below keep stay
            len = phys = x.index;
            const uint2 a = x.index >= 1 ? row[(uint32_t)(x.index - 1) & p.wmask] : make_uint2(0u, 0u);
            t1 = (int32_t)a.x;
            c1 = (int32_t)a.y;
            t2 = x.index >= 2 ? (int32_t)row[(uint32_t)(x.index - 2) & p.wmask].x : 0;
        }
        int32_t elec = q1.w;
        if (!keepv) {
            const u32x4 w = draw(p, t, (uint32_t)(p.g0 + x.g), RAFT_RNG_TIMER, (uint32_t)(x.r >> 2));
            elec = scale_range(word_of(w, x.r & 3), p.emin, p.emax);
        }
        *quad(p, 1, idx) = make_int4(len, phys, t1, elec);
        *quad(p, 2, idx) = make_int4(keepv ? q2.x : 0, t2, c1, keepv ? q2.w : 0);
    }
}

template <int R> struct ValidateL {
    static void run(raft_engine* e, const uint2* rec, int64_t n, unsigned long long* hdr) {
        replay_validate_kernel<R><<<(unsigned)((n + BLOCK - 1) / BLOCK), BLOCK, 0, e->stream>>>(e->dp, rec, n, hdr);
    }
};
template <int R> struct ApplyL {
    static void run(raft_engine* e, const uint2* rec, int64_t n, uint32_t flags) {
        replay_apply_kernel<R><<<(unsigned)((n + BLOCK - 1) / BLOCK), BLOCK, 0, e->stream>>>(e->dp, rec, n, (uint32_t)e->t,
                                                                                             flags);
    }
};

int replay(raft_engine* e, const raft_wal_record* rec, int64_t n, uint32_t flags, raft_replay_info* info, bool on_host) {
    if (!e) return raft_internal_fail(RAFT_EINVAL, "null engine");
    if (!info) return raft_internal_fail(RAFT_EINVAL, "null info");
    *info = raft_replay_info{};
    if (flags & ~(uint32_t)RAFT_REPLAY_KEEP_VOLATILE) return raft_internal_fail(RAFT_EINVAL, "unknown replay flag bits");
    if (int rc = check_args(e, n, !rec)) return rc;
    if (!on_host && ((uintptr_t)rec & 7u)) return raft_internal_fail(RAFT_EINVAL, "the record buffer must be 8-byte aligned");
    if (n == 0) return RAFT_OK;
    HIP_TRY(hipSetDevice(e->device));
    e->fork_needed = true;                           // later step launches wait for the replay
    if (int rc = raft_internal_grow_dev(e, &e->aux, &e->aux_bytes, ReplayTotals::BYTES)) return rc;
    ReplayTotals tot;
    if (int rc = tot.zero(e, e->aux)) return rc;
    const uint2* dev = (const uint2*)rec;
    if (on_host) {
        Staged s;
        const void* src[1] = {rec};
        const size_t bytes[1] = {(size_t)n * sizeof(raft_wal_record)};
        if (int rc = stage_in(e, src, bytes, 1, 0, s)) return rc;
        dev = (const uint2*)(e->cio + s.off[0]);
    }
    by_R<ValidateL>(e->p.R, e, dev, n, tot.dev);
    HIP_TRY(hipGetLastError());
    if (int rc = tot.fetch(e)) return rc;
    if (tot.w[RW_MALFORMED]) {                       // nothing was written
        info->malformed = (int64_t)tot.w[RW_MALFORMED];
        return raft_internal_fail(RAFT_EINVAL, std::to_string(info->malformed) + " malformed records: nothing was replayed");
    }
    by_R<ApplyL>(e->p.R, e, dev, n, flags);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(e->stream));
    info->applied = n;
    info->replicas = (int64_t)tot.w[RW_REPLICAS];
    info->hardstates = (int64_t)tot.w[RW_HS];
    info->truncates = (int64_t)tot.w[RW_TR];
    info->entries = (int64_t)tot.w[RW_EN];
    return RAFT_OK;
}

}  // namespace

extern "C" {

int raft_wal_replay(raft_engine* e, const raft_wal_record* rec_host, int64_t n, uint32_t flags, raft_replay_info* info) {
    return replay(e, rec_host, n, flags, info, true);
}

int raft_wal_replay_dev(raft_engine* e, const raft_wal_record* rec_dev, int64_t n, uint32_t flags, raft_replay_info* info) {
    return replay(e, rec_dev, n, flags, info, false);
}

}  // extern "C"
