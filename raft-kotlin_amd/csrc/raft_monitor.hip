// raft_monitor.hip — the liveness monitor (include/raft_engine.h raft_monitor_*):
// a ledger per group, in HBM of its own behind a handle of its own, that
// remembers since when the group has shown no leader, since when its leader's
// backlog has not advanced, where its churn window began and which replicas
// lag -- and an observe between two step launches that brings it up to date
// and says which groups make no progress now.  The safety audit's other half
// (raft_audit.hip): that one asks "did a group ever do something forbidden",
// this one "which groups are stuck, for how long, and why".  The reference has
// no counterpart.
//
// A side path with kernels of its own: observe reads quads 0, 1 and 2 of each
// replica (term and role, lastIndex, commitIndex) and no log slot, and writes
// only the ledger and the monitor's availability totals; report reads only
// the ledger.  Neither writes engine memory.
//   observe   the audit's shape: eight lanes per group (32 groups per
//             256-thread block), lane r < R is replica r.  Group-level
//             decisions go through __shfl_xor over the eight lanes and through
//             the group's byte of a ballot; the group's lead lane stores the
//             ledger, a quad only when it changed.  The counts of a call go
//             through ballots into a stripe (one atomic per nonzero word and
//             wave).  An outage that ended adds one to its bucket of the
//             histogram (one atomic per ended outage; they are rare), and a
//             wave in which some ended adds its two sums: integer adds only,
//             so any order gives the same totals.
//   report    the stream of raft_stream.h, as the audit's,
//             over the source "(now or ever) & kinds": 32-byte records in
//             group order.  Its scan and write run only when something is
//             delivered.
// The ledger on the device: four int4 per group at 4 g, the 16 words of
// raft_monitor_read in their order -- a wave's eight groups read one
// contiguous run of 512 bytes.
#include <hip/hip_runtime.h>

#include <climits>
#include <string>
#include <vector>

#include "raft_ledger.h"

using namespace raft;

struct raft_monitor : raft_ledger {   // mem: the ledger [G] of 64 bytes, then the availability totals, 256-byte aligned each
    raft_monitor_config cfg;
    int4* led;
    unsigned long long* avail;  // raft_monitor_availability as it lies: hist[32], outages, down_steps, reserved[2]
};

namespace {

static_assert(sizeof(raft_monitor_config) == 32 && sizeof(raft_monitor_info) == 96 && sizeof(raft_monitor_event) == 32 &&
                  sizeof(raft_monitor_report_info) == 64 && sizeof(raft_monitor_availability) == 288,
              "record layouts of the C-ABI");

constexpr int AVAIL_WORDS = sizeof(raft_monitor_availability) / 8, AV_OUTAGES = 32, AV_DOWN_STEPS = 33;
constexpr int LEDGER_WORDS = 16;

// the counts of an observe, striped as a restart's totals, at the head of aux; lines of 16 words
enum { MW_FLAGGED = 0, MW_NEWLY, MW_CLEARED, MW_LEADERLESS, MW_STALLED, MW_LAGGING, MW_CHURNING, MW_DOWN, MW_ENDED,
       MW_ENDED_STEPS, MW_WORDS };
constexpr int MON_LINE = 16;
using Counts = DevWords<unsigned long long, HDR_STRIPES, MON_LINE, MW_WORDS, true>;

// age(x) = max(0, (int32)(s - x)), the subtraction taken mod 2^32
__device__ __forceinline__ int32_t age(int32_t s, int32_t x) { return max(0, (int32_t)((uint32_t)s - (uint32_t)x)); }
__device__ __forceinline__ int32_t sat_add(int32_t a, int32_t b) {      // a, b >= 0
    return (int32_t)min((long long)a + b, (long long)INT_MAX);
}

__global__ __launch_bounds__(BLOCK) void monitor_fill_kernel(int4* __restrict__ led, int64_t g0, int64_t n) {
    const int64_t j = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j < n) {
        int4* L = led + 4 * (g0 + j);
        L[0] = make_int4(0, 0, 0, -1);
        L[1] = make_int4(-1, 0, 0, 0);
        L[2] = make_int4(-1, 0, -1, 0);
        L[3] = make_int4(0, 0, 0, 0);
    }
}

// One observe of groups [g0, g0 + n): the five rules of include/raft_engine.h,
// in their order.  Lanes of a group beyond R and groups beyond the range load
// at a clamped index, take part in the shuffles and store nothing.  Every lane
// of a group computes the group's new ledger; its lane 0 stores it.  The lanes
// past the range are clamped to the last group, g0 + n - 1, and may load its
// ledger quads while that group's lane 0 stores them: the race is tolerated,
// since nothing such a lane computes is used (head and end_h require live).
__global__ __launch_bounds__(BLOCK) void monitor_observe_kernel(DevParams p, raft_monitor_config cfg,
                                                                int4* __restrict__ led,
                                                                unsigned long long* __restrict__ avail, int64_t g0,
                                                                int64_t n, int32_t s, unsigned long long* cnt) {
    const int64_t j = ((int64_t)blockIdx.x * BLOCK + threadIdx.x) >> 3;
    const int r = threadIdx.x & 7, R = p.R;
    const bool live = j < n;
    const int64_t g = g0 + (live ? j : n - 1);                          // g0 <= g < g0 + n <= G (check_groups)
    const bool act = live && r < R;
    const int64_t idx = g * R + min(r, R - 1);
    const int4 q0 = *quad(p, 0, idx);                                   // term, votedFor, role
    const int32_t last = quad(p, 1, idx)->x;
    const int32_t commit = quad(p, 2, idx)->x;
    const int4 H0 = led[4 * g], H1 = led[4 * g + 1], H2 = led[4 * g + 2], H3 = led[4 * g + 3];   // one line per group
    const int32_t term = q0.x;
    const bool leader = act && q0.z == RAFT_LEADER;

    // the newest leader (find_newest_leader's rule: the highest term, the lowest index among equals), what it
    // shows, and the group's highest term
    const long long none = LLONG_MIN;
    const long long key = group_max64(leader ? (long long)term * 8 + (7 - r) : none);
    const int32_t L = key == none ? -1 : 7 - (int32_t)(key & 7);
    const int src = (threadIdx.x & 56) | max(L, 0);
    const int32_t last_L = __shfl(last, src, 64);
    const int32_t hi_L = __shfl(committed_hi(p, commit, last), src, 64);
    const int32_t T = group_max(act ? term : INT_MIN);
    uint32_t now = 0;

    // 1. outage
    int4 N1 = H1;
    bool ended = false;
    int32_t len = 0;
    if (L < 0) {
        if (N1.x == -1) N1.x = s;
        if (age(s, N1.x) >= cfg.leaderless_steps) now |= RAFT_MONITOR_LEADERLESS;
    } else if (H1.x != -1) {
        ended = true;
        len = max(1, age(s, H1.x));
        N1 = make_int4(-1, sat_add(H1.y, 1), sat_add(H1.z, len), max(H1.w, len));
    }

    // 2. stalled commit
    int4 N2 = H2;
    const bool backlog = L >= 0 && last_L > hi_L;
    if (!backlog) {
        N2.x = -1;
        N2.y = 0;
    } else {
        if (H2.x == -1 || hi_L > H2.y) {
            N2.x = s;
            N2.y = hi_L;
        }
        if (age(s, N2.x) >= cfg.stalled_steps) now |= RAFT_MONITOR_COMMIT_STALLED;
    }

    // 3. lag behind the newest leader
    const bool lag_on = cfg.lag_entries > 0 && L >= 0;
    const long long lag = (long long)last_L - last;
    const bool other = act && lag_on && r != L;
    const uint32_t lag_mask = group_bits(__ballot(other && lag >= cfg.lag_entries));
    const int32_t max_lag = group_max(other ? (int32_t)min(max(lag, 0ll), (long long)INT_MAX) : 0);
    if (lag_mask) now |= RAFT_MONITOR_LAGGING;
    const int4 N3 = make_int4((int32_t)lag_mask, max_lag, H3.z, H3.w);

    // 4. churn
    if (cfg.churn_terms > 0) {
        if (N2.z == -1) {
            N2.z = s;
            N2.w = T;
        }
        if ((long long)T - N2.w >= cfg.churn_terms) now |= RAFT_MONITOR_CHURNING;
        if (age(s, N2.z) >= cfg.churn_steps) {
            N2.z = s;
            N2.w = T;
        }
    }

    // 5. bookkeeping
    const uint32_t was = (uint32_t)H0.x, ever_was = (uint32_t)H0.y, ever = ever_was | now;
    const int4 N0 = make_int4((int32_t)now, (int32_t)ever, (ever_was == 0 && ever != 0) ? s : H0.z, L);
    const bool head = live && r == 0;
    if (head) {
        if (differ(N0, H0)) led[4 * g] = N0;
        if (differ(N1, H1)) led[4 * g + 1] = N1;
        if (differ(N2, H2)) led[4 * g + 2] = N2;
        if (differ(N3, H3)) led[4 * g + 3] = N3;
    }

    // availability: ended outages are rare
    const bool end_h = head && ended;
    if (end_h) atomicAdd(avail + (31 - __clz(len)), 1ull);             // len in 1..2^31-1: buckets 0..30
    const unsigned long long b_end = __ballot(end_h);
    unsigned long long steps = 0;
    if (b_end) {                                                        // wave-uniform
        steps = end_h ? (unsigned long long)len : 0ull;
        for (int o = 32; o > 0; o >>= 1) steps += __shfl_xor(steps, o, 64);
    }

    const unsigned long long b_fl = __ballot(head && now != 0), b_new = __ballot(head && was == 0 && now != 0),
                             b_clr = __ballot(head && was != 0 && now == 0),
                             b_ll = __ballot(head && (now & RAFT_MONITOR_LEADERLESS)),
                             b_st = __ballot(head && (now & RAFT_MONITOR_COMMIT_STALLED)),
                             b_lg = __ballot(head && (now & RAFT_MONITOR_LAGGING)),
                             b_ch = __ballot(head && (now & RAFT_MONITOR_CHURNING)),
                             b_dn = __ballot(head && N1.x != -1);
    if ((threadIdx.x & 63) == 0) {
        unsigned long long* line = stripe_of(cnt, wave_index(), MON_LINE);
        tally_ballot(line, MW_FLAGGED, b_fl);
        tally_ballot(line, MW_NEWLY, b_new);
        tally_ballot(line, MW_CLEARED, b_clr);
        tally_ballot(line, MW_LEADERLESS, b_ll);
        tally_ballot(line, MW_STALLED, b_st);
        tally_ballot(line, MW_LAGGING, b_lg);
        tally_ballot(line, MW_CHURNING, b_ch);
        tally_ballot(line, MW_DOWN, b_dn);
        tally_ballot(line, MW_ENDED, b_end);
        tally(line, MW_ENDED_STEPS, steps);
        if (b_end) {
            atomicAdd(avail + AV_OUTAGES, (unsigned long long)__popcll(b_end));
            atomicAdd(avail + AV_DOWN_STEPS, steps);
        }
    }
}

// the report's source (raft_stream.h): a group's first ledger quad, a record iff (now or ever) & kinds
struct MonitorSource {
    using Word = uint4;
    static constexpr int WORDS = 2, TALLIES = 1;                        // word 0: the groups listed
    struct Item {
        int4 H0;
        bool hit;
    };
    const int4* __restrict__ led;
    int32_t which, kinds;

    __device__ __forceinline__ Item eval(int64_t g, bool live) const {
        const int4 H0 = led[4 * g];
        return Item{H0, live && ((which == RAFT_MONITOR_EVER ? H0.y : H0.x) & kinds) != 0};
    }
    __device__ __forceinline__ void tallies(const Item& it, bool, unsigned long long (&b)[TALLIES]) const {
        b[0] = __ballot(it.hit);
    }
    __device__ __forceinline__ void record(const Item& it, int64_t g, uint4* st) const {
        const int32_t down = led[4 * g + 1].x, stall = led[4 * g + 2].x, lagm = led[4 * g + 3].x;
        st[0] = make_uint4((uint32_t)((uint64_t)g & 0xFFFFFFFFu), (uint32_t)((uint64_t)g >> 32), (uint32_t)it.H0.x,
                           (uint32_t)it.H0.y);
        st[1] = make_uint4((uint32_t)down, (uint32_t)stall, (uint32_t)it.H0.w, (uint32_t)lagm);
    }
    __device__ __forceinline__ void commit(const Item&, int64_t) const {}   // a report changes nothing
    static int64_t total(const unsigned long long* w) { return (int64_t)w[0]; }
};

int check_config(const raft_monitor_config* c) {
    if (!c) return raft_internal_fail(RAFT_EINVAL, "null config");
    if (c->leaderless_steps < 0 || c->stalled_steps < 0 || c->lag_entries < 0 || c->churn_terms < 0 || c->churn_steps < 0)
        return raft_internal_fail(RAFT_EINVAL, "a monitor threshold must be >= 0");
    if (c->churn_terms > 0 && c->churn_steps < 1)
        return raft_internal_fail(RAFT_EINVAL, "churn_steps must be >= 1 when churn_terms > 0");
    if (c->reserved[0] || c->reserved[1] || c->reserved[2])
        return raft_internal_fail(RAFT_EINVAL, "the config's reserved words must be 0");
    return RAFT_OK;
}

int report(raft_monitor* m, int64_t g0, int64_t n, int32_t which, int32_t kinds, raft_monitor_event* out,
           int64_t max_events, raft_monitor_report_info* info, bool out_on_host) {
    return ledger_report<MonitorSource>(m, "null monitor", g0, n, out, max_events, out_on_host, info, [&](MonitorSource& s) {
        if (which != RAFT_MONITOR_NOW && which != RAFT_MONITOR_EVER)
            return raft_internal_fail(RAFT_EINVAL, "which must be RAFT_MONITOR_NOW or RAFT_MONITOR_EVER");
        if ((uint32_t)kinds & ~(uint32_t)RAFT_MONITOR_ALL) return raft_internal_fail(RAFT_EINVAL, "kinds holds unknown bits");
        s = MonitorSource{m->led, which, kinds};
        return (int)RAFT_OK;
    });
}

}  // namespace

extern "C" {

int raft_monitor_create(raft_engine* e, const raft_monitor_config* cfg, raft_monitor** out) {
    if (int rc = create_args(e, out)) return rc;
    if (int rc = check_config(cfg)) return rc;
    const size_t led_b = al256((size_t)e->p.G * 64), av_b = al256(sizeof(raft_monitor_availability));
    return ledger_create(e, out, led_b + av_b, "the monitor's ledger", [&](raft_monitor* m) {
        m->cfg = *cfg;
        m->led = (int4*)m->mem;
        m->avail = (unsigned long long*)(m->mem + led_b);
        return raft_monitor_reset(m);
    });
}

int raft_monitor_destroy(raft_monitor* m) { return ledger_destroy(m); }

int raft_monitor_reset(raft_monitor* m) {
    return ledger_reset(m, "null monitor", [&](raft_engine* e) -> int {
        e->fork_needed = true;
        monitor_fill_kernel<<<grid_of(e->p.G), BLOCK, 0, e->stream>>>(m->led, 0, e->p.G);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemsetAsync(m->avail, 0, sizeof(raft_monitor_availability), e->stream));
        return RAFT_OK;
    });
}

int64_t raft_monitor_device_bytes(raft_monitor* m) { return ledger_bytes(m); }

int raft_monitor_observe(raft_monitor* m, int64_t g0, int64_t n, raft_monitor_info* info) {
    Counts c{};
    if (int rc = ledger_observe(m, "null monitor", g0, n, info, c, [&](unsigned grid, unsigned long long* cnt) {
            monitor_observe_kernel<<<grid, BLOCK, 0, m->e->stream>>>(m->e->dp, m->cfg, m->led, m->avail, g0, n,
                                                                     (int32_t)(uint32_t)m->e->t, cnt);
        }))
        return rc;
    info->flagged = (int64_t)c.w[MW_FLAGGED];
    info->newly_flagged = (int64_t)c.w[MW_NEWLY];
    info->cleared = (int64_t)c.w[MW_CLEARED];
    info->leaderless = (int64_t)c.w[MW_LEADERLESS];
    info->commit_stalled = (int64_t)c.w[MW_STALLED];
    info->lagging = (int64_t)c.w[MW_LAGGING];
    info->churning = (int64_t)c.w[MW_CHURNING];
    info->down = (int64_t)c.w[MW_DOWN];
    info->outages_ended = (int64_t)c.w[MW_ENDED];
    info->down_steps_ended = (int64_t)c.w[MW_ENDED_STEPS];
    return RAFT_OK;
}

int raft_monitor_report(raft_monitor* m, int64_t g0, int64_t n, int32_t which, int32_t kinds,
                        raft_monitor_event* out_host, int64_t max_events, raft_monitor_report_info* info) {
    return report(m, g0, n, which, kinds, out_host, max_events, info, true);
}

int raft_monitor_report_dev(raft_monitor* m, int64_t g0, int64_t n, int32_t which, int32_t kinds,
                            raft_monitor_event* out_dev, int64_t max_events, raft_monitor_report_info* info) {
    return report(m, g0, n, which, kinds, out_dev, max_events, info, false);
}

// the availability totals are one row of the handle, not of a group: its own null word, no fork_needed on a set
int raft_monitor_get_availability(raft_monitor* m, raft_monitor_availability* out) {
    if (int rc = check_ledger(m, 0, 0, "null monitor")) return rc;
    if (!out) return raft_internal_fail(RAFT_EINVAL, "null availability");
    return rows_out(m->e, m->avail, sizeof(*out), out);
}

int raft_monitor_set_availability(raft_monitor* m, const raft_monitor_availability* in) {
    if (int rc = check_ledger(m, 0, 0, "null monitor")) return rc;
    if (!in) return raft_internal_fail(RAFT_EINVAL, "null availability");
    const int64_t* w = (const int64_t*)in;
    for (int i = 0; i < AVAIL_WORDS; ++i)
        if (w[i] < 0) return raft_internal_fail(RAFT_EINVAL, "an availability total must be >= 0");
    if (in->reserved[0] || in->reserved[1]) return raft_internal_fail(RAFT_EINVAL, "the reserved words must be 0");
    return rows_in(m->e, m->avail, in, sizeof(*in));
}

int raft_monitor_read(raft_monitor* m, int64_t g0, int64_t n, int32_t* out) {
    return table_call(check_ledger(m, g0, n, "null monitor"), n, out,
                      [&] { return rows_out(m->e, m->led + 4 * g0, (size_t)n * 64, out); });
}

int raft_monitor_write(raft_monitor* m, int64_t g0, int64_t n, const int32_t* in) {
    return table_call(check_ledger(m, g0, n, "null monitor"), n, in, [&]() -> int {
        const int R = m->e->p.R;
        for (int64_t k = 0; k < n; ++k) {
            const int32_t* w = in + k * LEDGER_WORDS;
            if (((uint32_t)w[0] | (uint32_t)w[1]) & ~(uint32_t)RAFT_MONITOR_ALL)
                return raft_internal_fail(RAFT_EINVAL, "a ledger's now or ever holds unknown bits");
            if (w[3] < -1 || w[3] >= R) return raft_internal_fail(RAFT_EINVAL, "a ledger's leader must be in -1..R-1");
            if ((uint32_t)w[12] >> R) return raft_internal_fail(RAFT_EINVAL, "a ledger's lag_mask holds bits at or above R");
            if (w[5] < 0 || w[6] < 0 || w[7] < 0 || w[13] < 0 || w[9] < 0)
                return raft_internal_fail(RAFT_EINVAL,
                                          "a ledger's outages, down_total, longest, max_lag and stall_mark must be >= 0");
            if (w[14] || w[15]) return raft_internal_fail(RAFT_EINVAL, "a ledger's reserved words must be 0");
        }
        m->e->fork_needed = true;
        return rows_in(m->e, m->led + 4 * g0, in, (size_t)n * 64);
    });
}

}  // extern "C"
