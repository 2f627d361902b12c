// raft_wal.hip — the persistence stream (include/raft_engine.h raft_wal_*):
// what a replica must make durable before its answers count -- currentTerm,
// votedFor and the log entries it gained or replaced since the last poll
// (etcd's Ready.HardState and Ready.Entries) -- as an ordered delta stream.
// The drain (raft_apply.hip) hands out what became committed; this hands out
// what became part of the log, committed or not, and says when a part that
// was handed out is no longer the replica's log.  The reference persists
// nothing and has no counterpart.
//
// A side path with kernels of its own behind a handle of its own: it reads
// quads 0, 1 and 2 of each selected replica and log slots, and writes only
// the handle's cursors and the caller's record buffer.  It never writes engine
// memory.  Three passes on the engine stream, in the drain's shape:
//   1. count   one thread per selected replica: the rule of the header (hard
//              state changed? still clean? how many entries?) from the state
//              quads, the cursor and at most one log slot (stable - 1).  Stores
//              the replica's record count and, beside it, a 2-bit word "has
//              HARDSTATE / has TRUNCATE"; lost, regressed and the per-kind
//              totals go into a stripe, one atomic per wave and nonzero word
//   2. scan    exclusive scan of the counts (rocprim, ScanScratch)
//   3. expand  balanced by output slot: a wave owns 64 consecutive replicas
//              and walks their output range 64 slots at a time; each lane
//              finds its slot's owner by apply_expand_kernel's shuffle binary
//              search, maps the slot's rank inside the owner's run to a kind
//              (HARDSTATE, TRUNCATE, then ENTRY ascending), reads one 8-byte
//              log slot for an ENTRY and stages the 24-byte record in the
//              wave's LDS slice; wave_publish<3> stores them contiguously.
//              After the loop each replica's owner lane writes its cursor,
//              once, past exactly what was written.  It runs on every poll
//              that is not a peek, also when nothing is delivered: the floors
//              of the clean replicas follow their commit points.
// Why no shadow log is needed (the argument is in the header and DESIGN.md
// §4.22): Log Matching makes one term comparison at stable - 1 a proof that
// the whole handed-out prefix is still the replica's log, and a replica's own
// committed prefix [0, floor) never changes in textbook mode, so re-sending
// from floor after any mismatch is always enough.
//
// The cursor on the device is the export form as it lies: three uint2 per
// replica at 3 (g R + r) -- (term, vote), (stable, stable_term), (floor, pad).
// The staging (counts, flags, offsets, scan scratch, the device copy of a host
// poll's records) is the drain's grow-only staging of the engine: the calls
// are serialised on the engine stream and return after their kernels.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "raft_ledger.h"

using namespace raft;

struct raft_wal : raft_ledger {   // mem: the cursors [G * R] of 24 bytes
    uint2* cur;
};

namespace {

static_assert(sizeof(raft_wal_cursor) == 24 && sizeof(raft_wal_record) == 24 && sizeof(raft_wal_info) == 56,
              "record layouts of the C-ABI");

// the totals of a poll, striped: what the count pass found, and (only when the
// room cuts the stream) what the expand pass wrote
enum { WW_LOST = 0, WW_REGRESSED, WW_HS, WW_TR, WW_EN, WW_WROTE_HS, WW_WROTE_TR, WW_WROTE_EN, WW_WORDS };
using WalTotals = DevWords<unsigned long long, HDR_STRIPES, HDR_LINE, WW_WORDS, true>;
constexpr uint32_t HAS_HS = 1u, HAS_TR = 2u;

// the log row of replica idx = g * R + r (log_of with a compile-time R)
template <int R>
__device__ __forceinline__ const uint2* row_of(const DevParams& p, int64_t idx) {
    constexpr int GPW = 64 / R;
    const int64_t g = idx / R, w = g / GPW;
    return p.log + (w * 64 + ((g - w * GPW) * R + (idx - g * R))) * (int64_t)p.nslots;
}

// One replica against its cursor: the rule of include/raft_engine.h.
struct Plan {
    int32_t last, hi;           // lastIndex and the committed prefix, both within 0..log_cap
    int32_t wl;                 // the first readable index (0 on a flat log)
    int32_t from;               // stable after a TRUNCATE (keep), else the cursor's
    int32_t first;              // the first entry sent: from, or the window's low end above it
    uint32_t flags;             // HAS_HS | HAS_TR
    bool regressed;
};
// term of entry i - 1, 0 when i == 0 or the slot left the window; i <= log_cap
__device__ __forceinline__ int32_t term_before(const DevParams& p, const uint2* row, int32_t i, int32_t wl) {
    return i > 0 && i - 1 >= wl ? (int32_t)row[(uint32_t)(i - 1) & p.wmask].x : 0;
}
__device__ __forceinline__ Plan plan_of(const DevParams& p, const uint2* row, int4 q0, int4 q1, int32_t commit, uint2 c0,
                                        uint2 c1, uint2 c2, bool probe, uint32_t known) {
    Plan pl;
    pl.last = max(0, min(q1.x, p.cap));
    pl.hi = committed_hi(p, commit, q1.x);
    pl.wl = p.W != FLAT_W ? max(0, q1.y - p.W) : 0;
    const int32_t stable = (int32_t)c1.x, floor_ = (int32_t)c2.x;
    uint32_t fl = (q0.x != (int32_t)c0.x || q0.y != (int32_t)c0.y) ? HAS_HS : 0u;
    if (probe) {                                                       // the count pass decides, the expand pass is told
        bool clean = stable <= pl.last;
        if (clean && stable > 0)                                       // stable - 1 < lastIndex <= log_cap: inside the row
            clean = stable - 1 >= pl.wl && (int32_t)row[(uint32_t)(stable - 1) & p.wmask].x == (int32_t)c1.y;
        fl |= clean ? 0u : HAS_TR;
    } else {
        fl = known;
    }
    pl.flags = fl;
    const int32_t keep = min(floor_, pl.last);
    pl.regressed = (fl & HAS_TR) && keep < floor_;
    pl.from = (fl & HAS_TR) ? keep : stable;
    pl.first = max(pl.from, min(pl.wl, pl.last));                      // from <= last: first is within from..last
    return pl;
}

__global__ __launch_bounds__(BLOCK) void wal_fill_kernel(uint2* __restrict__ cur, int64_t n) {
    const int64_t j = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j < n) {
        cur[3 * j + 0] = make_uint2(0u, (uint32_t)-1);                 // term 0, vote -1
        cur[3 * j + 1] = make_uint2(0u, 0u);
        cur[3 * j + 2] = make_uint2(0u, 0u);
    }
}

// pass 1.  cnt[j]: records replica j of the selection has to send, cnt[N] = 0
// (the scan's last element is then the total); flg[j]: its HAS_* bits.
template <int R>
__global__ __launch_bounds__(BLOCK) void wal_count_kernel(DevParams p, const uint2* __restrict__ cur, Sel s,
                                                          uint32_t* __restrict__ cnt, uint8_t* __restrict__ flg,
                                                          unsigned long long* hdr) {
    const int64_t j = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    uint32_t lost = 0, entries = 0, flags = 0;
    bool regressed = false;
    if (j < s.N) {
        const int64_t idx = sel_idx<R>(s, j);
        const Plan pl = plan_of(p, row_of<R>(p, idx), *quad(p, 0, idx), *quad(p, 1, idx), quad(p, 2, idx)->x, cur[3 * idx],
                                cur[3 * idx + 1], cur[3 * idx + 2], true, 0u);
        flags = pl.flags;
        regressed = pl.regressed;
        lost = (uint32_t)(pl.first - pl.from);
        entries = (uint32_t)(pl.last - pl.first);
        cnt[j] = entries + (flags & 1u) + (flags >> 1);
        flg[j] = (uint8_t)flags;
    } else if (j == s.N) {
        cnt[j] = 0u;
    }
    // one atomic per wave and nonzero word (a run is < 2^23: a wave's sum fits 32 bits)
    const uint32_t wl = wave_sum(lost), we = wave_sum(entries);
    const unsigned long long b_rg = __ballot(regressed), b_hs = __ballot(flags & HAS_HS), b_tr = __ballot(flags & HAS_TR);
    if ((threadIdx.x & 63) == 0) {
        unsigned long long* line = stripe_of(hdr, wave_index());
        tally(line, WW_LOST, wl);
        tally(line, WW_EN, we);
        tally_ballot(line, WW_REGRESSED, b_rg);
        tally_ballot(line, WW_HS, b_hs);
        tally_ballot(line, WW_TR, b_tr);
    }
}

// pass 3.  Wave w of the grid owns replicas [64 w, 64 w + 64) of the selection
// and their output slots [off[64 w], off[64 w + 64)), cut at max_records.  hdr
// is null unless the room cuts the stream: then the kinds written are tallied.
template <int R>
__global__ __launch_bounds__(BLOCK) void wal_expand_kernel(DevParams p, uint2* __restrict__ cur, Sel s,
                                                           const uint32_t* __restrict__ cnt,
                                                           const uint8_t* __restrict__ flg,
                                                           const unsigned long long* __restrict__ off,
                                                           uint2* __restrict__ out, int64_t max_records,
                                                           unsigned long long* hdr) {
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
    const uint2* my_row = row_of<R>(p, my_idx);
    const int4 q0 = *quad(p, 0, my_idx);
    const uint2 c0 = cur[3 * my_idx], c1 = cur[3 * my_idx + 1], c2 = cur[3 * my_idx + 2];
    const Plan pl = plan_of(p, my_row, q0, *quad(p, 1, my_idx), quad(p, 2, my_idx)->x, c0, c1, c2, false,
                            mine ? (uint32_t)flg[j] : 0u);
    const uint32_t hs = pl.flags & 1u, tr = pl.flags >> 1;
    const unsigned long long base = __shfl(my_off, 0, 64);
    const unsigned long long room = (unsigned long long)max_records;
    // offsets inside the tile fit 32 bits (64 replicas of < 2^23 + 2 slots); the
    // lanes past the selection carry the tile's end, so the search never picks them
    const uint32_t roff = (uint32_t)(my_off - base);
    const uint32_t span = __shfl(roff + my_cnt, 63, 64);
    const uint32_t end = base < room ? (uint32_t)min((unsigned long long)span, room - base) : 0u;
    // what a slot's record needs from its owner, fetched by shuffle: (group - the tile's first group, the HAS_*
    // bits, replica) in one word (G < 2^31, at most 64 groups a tile), and the first entry's index
    const int32_t g = (int32_t)(my_idx / R);
    const int32_t gw = __shfl(g, 0, 64);
    const int32_t pk = (g - gw) << 5 | (int32_t)pl.flags << 3 | (int32_t)(my_idx - (int64_t)g * R);
    const bool any_head = __ballot(pl.flags != 0) != 0;                 // wave-uniform: some run starts with a head record
    constexpr int GPW = 64 / R;
    uint2* st = stage[wv];
    uint32_t n_hs = 0, n_tr = 0, n_en = 0;                              // wave-uniform: written, per kind
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
        const int32_t opk = __shfl(pk, k, 64);
        const int32_t ofirst = __shfl(pl.first, k, 64);
        int32_t oterm = 0, ovote = 0, okeep = 0;
        if (any_head) {                                                // every lane takes part in the shuffles
            oterm = __shfl(q0.x, k, 64);
            ovote = __shfl(q0.y, k, 64);
            okeep = __shfl(pl.from, k, 64);
        }
        const int32_t og = gw + (opk >> 5), orr = opk & 7;
        const uint32_t ohs = (uint32_t)(opk >> 3) & 1u, otr = (uint32_t)(opk >> 4) & 1u;
        const uint32_t rank = x - rk;                                  // inside the owner's run
        const int kind = rank < ohs ? RAFT_WAL_HARDSTATE : rank < ohs + otr ? RAFT_WAL_TRUNCATE : RAFT_WAL_ENTRY;
        if (live) {
            uint2 w1, w2;
            if (kind == RAFT_WAL_ENTRY) {
                // the owner's log row: index < its lastIndex <= log_cap, inside the row
                const int32_t index = ofirst + (int32_t)(rank - ohs - otr);
                const int32_t w = og / GPW;
                const uint2* row = p.log + ((int64_t)w * 64 + ((og - w * GPW) * R + orr)) * (int64_t)p.nslots;
                const uint2 e = row[(uint32_t)index & p.wmask];
                w1 = make_uint2((uint32_t)index, e.x);                 // (term, cmd) as the log holds them
                w2 = make_uint2(e.y, 0u);
            } else if (kind == RAFT_WAL_HARDSTATE) {
                w1 = make_uint2((uint32_t)-1, (uint32_t)oterm);
                w2 = make_uint2(0u, (uint32_t)ovote);
            } else {
                w1 = make_uint2((uint32_t)okeep, 0u);
                w2 = make_uint2(0u, 0u);
            }
            st[3 * lane + 0] = make_uint2((uint32_t)og, (uint32_t)orr | (uint32_t)kind << 16);
            st[3 * lane + 1] = w1;
            st[3 * lane + 2] = w2;
        }
        if (hdr) {                                                     // uniform: the room cuts the stream
            n_hs += (uint32_t)__popcll(__ballot(live && kind == RAFT_WAL_HARDSTATE));
            n_tr += (uint32_t)__popcll(__ballot(live && kind == RAFT_WAL_TRUNCATE));
            n_en += (uint32_t)__popcll(__ballot(live && kind == RAFT_WAL_ENTRY));
        }
        wave_publish<3>(st, out + (base + x0) * 3, 3 * min(64u, end - x0));
        wave_lds_fence();                                              // the next trip stages into st again
    }
    if (hdr && lane == 0) {
        unsigned long long* line = stripe_of(hdr, j0 >> 6);
        tally(line, WW_WROTE_HS, n_hs);
        tally(line, WW_WROTE_TR, n_tr);
        tally(line, WW_WROTE_EN, n_en);
    }
    // the cursor moves past what was written, once per replica
    if (mine) {
        const unsigned long long left = my_off < room ? room - my_off : 0ull;
        const uint32_t wrote = (uint32_t)min((unsigned long long)my_cnt, left);
        const bool w_hs = hs && wrote >= 1u, w_tr = tr && wrote > hs;
        const uint32_t w_en = wrote > hs + tr ? wrote - hs - tr : 0u;
        const int32_t stable = w_en ? pl.first + (int32_t)w_en : w_tr ? pl.from : (int32_t)c1.x;
        const uint2 n0 = w_hs ? make_uint2((uint32_t)q0.x, (uint32_t)q0.y) : c0;
        uint2 n1 = c1, n2 = c2;
        if (w_tr || w_en) n1 = make_uint2((uint32_t)stable, (uint32_t)term_before(p, my_row, stable, pl.wl));
        if (!tr || w_tr) n2.x = (uint32_t)min(pl.hi, stable);          // the handed-out prefix is the replica's log
        if (n0.x != c0.x || n0.y != c0.y) cur[3 * my_idx] = n0;
        if (n1.x != c1.x || n1.y != c1.y) cur[3 * my_idx + 1] = n1;
        if (n2.x != c2.x) cur[3 * my_idx + 2] = n2;
    }
}

template <int R> struct CountW {
    static void run(raft_engine* e, const uint2* cur, const Sel& s, uint32_t* cnt, uint8_t* flg, unsigned long long* hdr) {
        wal_count_kernel<R><<<grid_of(s.N + 1), BLOCK, 0, e->stream>>>(e->dp, cur, s, cnt, flg, hdr);
    }
};
template <int R> struct ExpandW {
    static void run(raft_engine* e, uint2* cur, const Sel& s, const uint32_t* cnt, const uint8_t* flg,
                    const unsigned long long* off, uint2* out, int64_t max_records, unsigned long long* hdr) {
        const int64_t tiles = (s.N + 63) / 64;
        const unsigned grid = (unsigned)((tiles + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK);
        wal_expand_kernel<R><<<grid, BLOCK, 0, e->stream>>>(e->dp, cur, s, cnt, flg, off, out, max_records, hdr);
    }
};

int poll(raft_wal* w, int64_t g0, int64_t n, int32_t replica, raft_wal_record* out, int64_t max_records,
         raft_wal_info* info, bool out_on_host) {
    if (!w || !w->e) return raft_internal_fail(RAFT_EINVAL, "null wal");
    if (!info) return raft_internal_fail(RAFT_EINVAL, "null info");
    *info = raft_wal_info{};
    raft_engine* e = w->e;
    if (int rc = check_groups(e, g0, n)) return rc;
    if (replica < -1 || replica >= e->p.R) return raft_internal_fail(RAFT_EINVAL, "replica must be -1 or in 0..R-1");
    if (int rc = check_records(out, max_records, out_on_host, 8, "max_records")) return rc;
    if (n == 0) return RAFT_OK;
    const bool peek = !out && max_records == 0;
    HIP_TRY(hipSetDevice(e->device));
    e->fork_needed = true;                           // later step launches wait for these reads of the state and logs
    const Sel s{g0, replica < 0 ? n * e->p.R : n, replica};
    ScanScratch<uint32_t> sc;                        // one item per selected replica and the zero behind them
    const size_t flg_b = al256((size_t)s.N);
    if (int rc = sc.init(e, &e->apl, &e->apl_bytes, WalTotals::BYTES + flg_b, (size_t)s.N + 1)) return rc;
    uint8_t* flg = (uint8_t*)(sc.head + WalTotals::BYTES);
    WalTotals t;
    if (int rc = t.zero(e, sc.head)) return rc;
    by_R<CountW>(e->p.R, e, (const uint2*)w->cur, s, sc.cnt, flg, t.dev);
    HIP_TRY(hipGetLastError());
    if (int rc = t.fetch(e)) return rc;
    const int64_t total = (int64_t)(t.w[WW_HS] + t.w[WW_TR] + t.w[WW_EN]);
    const int64_t delivered = peek ? 0 : std::min(total, max_records);
    const bool cut = delivered < total;
    info->delivered = delivered;
    info->pending = total - delivered;
    info->lost = (int64_t)t.w[WW_LOST];
    info->regressed = (int64_t)t.w[WW_REGRESSED];
    if (!peek) {
        Records rec;
        if (int rc = rec.begin(e, out, (size_t)delivered * sizeof(raft_wal_record), out_on_host)) return rc;
        if (int rc = sc.run(e)) return rc;
        by_R<ExpandW>(e->p.R, e, w->cur, s, sc.cnt, flg, sc.off, (uint2*)rec.dev, max_records, cut ? t.dev : nullptr);
        HIP_TRY(hipGetLastError());
        if (cut)
            if (int rc = t.fetch(e)) return rc;
        if (int rc = rec.finish(e)) return rc;
        info->hardstates = (int64_t)t.w[cut ? WW_WROTE_HS : WW_HS];
        info->truncates = (int64_t)t.w[cut ? WW_WROTE_TR : WW_TR];
        info->entries = (int64_t)t.w[cut ? WW_WROTE_EN : WW_EN];
    }
    if (info->lost > 0)
        return raft_internal_fail(RAFT_EWINDOW, std::to_string(info->lost) +
                                                    " log entries left the log window unpersisted (skipped)");
    return RAFT_OK;
}

}  // namespace

extern "C" {

int raft_wal_create(raft_engine* e, raft_wal** out) {
    if (int rc = create_args(e, out)) return rc;
    return ledger_create(e, out, al256((size_t)e->dp.GR * sizeof(raft_wal_cursor)), "the wal's cursors", [](raft_wal* w) {
        w->cur = (uint2*)w->mem;
        return raft_wal_reset(w);
    });
}

int raft_wal_destroy(raft_wal* w) { return ledger_destroy(w); }

int raft_wal_reset(raft_wal* w) {
    return ledger_reset(w, "null wal", [&](raft_engine* e) -> int {
        e->fork_needed = true;
        wal_fill_kernel<<<grid_of(e->dp.GR), BLOCK, 0, e->stream>>>(w->cur, e->dp.GR);
        HIP_TRY(hipGetLastError());
        return RAFT_OK;
    });
}

int64_t raft_wal_device_bytes(raft_wal* w) { return ledger_bytes(w); }

int raft_wal_poll(raft_wal* w, int64_t g0, int64_t n, int32_t replica, raft_wal_record* out_host, int64_t max_records,
                  raft_wal_info* info) {
    return poll(w, g0, n, replica, out_host, max_records, info, true);
}

int raft_wal_poll_dev(raft_wal* w, int64_t g0, int64_t n, int32_t replica, raft_wal_record* out_dev,
                      int64_t max_records, raft_wal_info* info) {
    return poll(w, g0, n, replica, out_dev, max_records, info, false);
}

// replicas are indexed g * R + r: a range of groups is one contiguous run of cursors
int raft_wal_read(raft_wal* w, int64_t g0, int64_t n, raft_wal_cursor* cursors) {
    return table_call(check_ledger(w, g0, n, "null wal"), n, cursors, [&] {
        const int64_t R = w->e->p.R;
        return rows_out(w->e, w->cur + 3 * g0 * R, (size_t)(n * R) * sizeof(raft_wal_cursor), cursors);
    });
}

int raft_wal_write(raft_wal* w, int64_t g0, int64_t n, const raft_wal_cursor* cursors) {
    return table_call(check_ledger(w, g0, n, "null wal"), n, cursors, [&]() -> int {
        raft_engine* e = w->e;
        for (int64_t k = 0; k < n * e->p.R; ++k) {   // a poll reads log slots [stable - 1, lastIndex): keep it inside the row
            const raft_wal_cursor& c = cursors[k];
            const char* why = c.stable < 0 || c.stable > e->p.log_cap ? "a cursor's stable must be in 0..log_cap"
                              : c.floor < 0 || c.floor > c.stable   ? "a cursor's floor must be in 0..stable"
                              : c.vote < -1 || c.vote > e->p.R      ? "a cursor's vote must be in -1..R"
                              : c.term < 0                          ? "a cursor's term must be >= 0"
                              : c.pad                               ? "a cursor's pad must be 0"
                                                                    : nullptr;
            if (why) return raft_internal_fail(RAFT_EINVAL, why);
        }
        e->fork_needed = true;
        return rows_in(e, w->cur + 3 * g0 * e->p.R, cursors, (size_t)n * e->p.R * sizeof(raft_wal_cursor));
    });
}

}  // extern "C"
