// raft_audit.hip — the safety audit (include/raft_engine.h raft_audit_*): a
// ledger per group, in HBM of its own behind a handle of its own, that
// remembers what the group has shown -- every replica's (currentTerm,
// votedFor), the newest leader seen, the longest committed prefix seen and the
// entry at its end -- and an observe between two step launches that checks
// the state now against it: a term that went backwards, a vote changed within
// a term, two leaders of one term (at once, or across two observes), a
// committed entry that changed, a newer leader that lacks it.  The reference
// has no counterpart.
//
// A side path with kernels of its own: observe reads quads 0 and 1 and
// commitIndex of each replica and at most two 8-byte log slots per group, and
// writes only the ledger; report reads only the ledger.  Neither writes engine
// memory.
//   observe   eight lanes per group (raft_ticket.h's shape: 32 groups per
//             256-thread block), lane r < R is replica r.  Group-level
//             decisions go through __shfl_xor over the eight lanes and through
//             the group's byte of a ballot; lane 0 stores the header.  The
//             counts of a call go through ballots into a stripe (one atomic per
//             nonzero word and wave).
//   report    the stream of raft_stream.h, as the leader
//             watch's, over the source "flags != 0": 16-byte records in group
//             order.  Its scan and write run only when something is delivered.
// The ledger on the device: hdr, two int4 per group (flags, first_step,
// lead_term, lead_replica | anchor_count, anchor_term, anchor_cmd,
// anchor_seen_term), and pairs, one int2 (currentTerm, votedFor) per replica at
// g * R + r -- a wave's 32 groups read one contiguous run of each.
#include <hip/hip_runtime.h>

#include <climits>
#include <string>
#include <vector>

#include "raft_ledger.h"

using namespace raft;

struct raft_audit : raft_ledger {   // mem: hdr [G] of 32 bytes, then pairs [G * R] of 8 bytes, 256-byte aligned each
    int4* hdr;
    int2* pairs;
};

namespace {

static_assert(sizeof(raft_audit_event) == 16 && sizeof(raft_audit_info) == 64 && sizeof(raft_audit_report_info) == 64,
              "record layouts of the C-ABI");

constexpr uint32_t AUDIT_ALL = RAFT_AUDIT_TERM_REGRESSED | RAFT_AUDIT_VOTE_CHANGED | RAFT_AUDIT_TWO_LEADERS |
                               RAFT_AUDIT_COMMIT_CHANGED | RAFT_AUDIT_LEADER_INCOMPLETE;

// the counts of an observe, striped as a restart's totals, at the head of aux; a report uses word 0 alone
enum { AW_NEWLY = 0, AW_FLAGGED, AW_TERM, AW_VOTE, AW_TWO, AW_COMMIT, AW_LEADER, AW_UNKNOWN, AW_WORDS };
using Counts = DevWords<unsigned long long, HDR_STRIPES, HDR_LINE, AW_WORDS, true>;

__global__ __launch_bounds__(BLOCK) void audit_fill_kernel(int4* __restrict__ hdr, int2* __restrict__ pairs, int64_t g0,
                                                           int64_t n, int R) {
    const int64_t j = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j < n) {
        hdr[2 * (g0 + j)] = make_int4(0, 0, 0, -1);
        hdr[2 * (g0 + j) + 1] = make_int4(0, 0, 0, 0);
    }
    if (j < n * R) pairs[g0 * R + j] = make_int2(0, -1);
}

// One observe of groups [g0, g0 + n): the five steps of include/raft_engine.h,
// in their order.  Lanes of a group beyond R and groups beyond the range load
// at a clamped index, take part in the shuffles and store nothing.
__global__ __launch_bounds__(BLOCK) void audit_observe_kernel(DevParams p, int4* __restrict__ hdr,
                                                              int2* __restrict__ pairs, int64_t g0, int64_t n,
                                                              int32_t step, unsigned long long* cnt) {
    const int64_t j = ((int64_t)blockIdx.x * BLOCK + threadIdx.x) >> 3;
    const int r = threadIdx.x & 7, R = p.R;
    const bool live = j < n;
    const int64_t g = g0 + (live ? j : n - 1);                          // g0 <= g < g0 + n <= G (check_groups)
    const bool act = live && r < R;
    const int64_t idx = g * R + min(r, R - 1);
    const int4 q0 = *quad(p, 0, idx);                                   // term, votedFor, role
    const int4 q1 = *quad(p, 1, idx);                                   // lastIndex, physLen
    const int32_t commit = quad(p, 2, idx)->x;
    const int2 old = pairs[idx];
    const int4 H0 = hdr[2 * g], H1 = hdr[2 * g + 1];                    // the group's eight lanes read one sector
    const int32_t term = q0.x, voted = q0.y, last = q1.x, phys = q1.y;
    const bool leader = act && q0.z == RAFT_LEADER;
    const bool ring = p.W != FLAT_W;
    uint32_t bits = 0;

    // 1. term and vote
    if (act && term < old.x) bits |= RAFT_AUDIT_TERM_REGRESSED;
    if (act && term == old.x && old.y >= 0 && voted != old.y) bits |= RAFT_AUDIT_VOTE_CHANGED;
    if (act && (term != old.x || voted != old.y)) pairs[idx] = make_int2(term, voted);

    // 2. Election Safety: now, and against the leader on record
    const uint32_t lbits = group_bits(__ballot(leader));
    bool twin = false;
#pragma unroll
    for (int d = 1; d < 8; ++d) {
        const int32_t to = __shfl_xor(term, d, 64);
        twin |= ((lbits >> (r ^ d)) & 1u) && to == term;
    }
    if (leader && (twin || (term == H0.z && H0.w >= 0 && r != H0.w))) bits |= RAFT_AUDIT_TWO_LEADERS;
    // find_newest_leader's rule: the highest term, the lowest index among equals
    const long long none = LLONG_MIN;
    const long long key = group_max64(leader ? (long long)term * 8 + (7 - r) : none);
    int32_t lead_term = H0.z, lead_rep = H0.w;
    if (key != none && (int32_t)(key >> 3) > lead_term) {
        lead_term = (int32_t)(key >> 3);
        lead_rep = 7 - (int32_t)(key & 7);
    }

    // 3. the anchor: slot C - 1, read only after the bounds and window tests
    const int32_t C = H1.x, hi = committed_hi(p, commit, last);
    bool unk_a = false, unk_b = false;
    if (C > 0) {
        const int32_t i = C - 1;
        const bool below = ring && i < phys - p.W;
        const bool need_a = act && hi >= C;                             // (then i < lastIndex)
        const bool newer = leader && term > H1.w;
        const bool need_b = newer && last >= C;
        if (newer && last < C) bits |= RAFT_AUDIT_LEADER_INCOMPLETE;
        unk_a = need_a && below;
        unk_b = need_b && below;
        if ((need_a || need_b) && !below && i < p.cap) {
            const uint2 en = *log_of(p, idx).at<true>(i);
            if ((int32_t)en.x != H1.y || en.y != (uint32_t)H1.z)
                bits |= (need_a ? RAFT_AUDIT_COMMIT_CHANGED : 0u) | (need_b ? RAFT_AUDIT_LEADER_INCOMPLETE : 0u);
        }
    }

    // 4. advance: the second slot read only in the one lane of a group that advances
    const int32_t Cn = group_max(act ? hi : 0);
    const bool adv = Cn > C;
    const uint32_t hbits = group_bits(__ballot(act && hi == Cn));
    const int rs = hbits ? __ffs(hbits) - 1 : 0;
    const bool mine = adv && act && r == rs;
    const bool below_n = ring && Cn - 1 < phys - p.W;
    uint2 en2 = make_uint2(0u, 0u);
    if (mine && !below_n) en2 = *log_of(p, idx).at<true>(Cn - 1);       // Cn - 1 < hi <= min(lastIndex, log_cap)
    const bool unk_n = mine && below_n;
    const int32_t seen_term = group_max(act ? term : INT_MIN);
    const int src = (threadIdx.x & 56) | rs;
    const uint32_t e2t = __shfl(en2.x, src, 64), e2c = __shfl(en2.y, src, 64);
    const bool skip = __shfl((int)below_n, src, 64) != 0;
    int4 N1 = H1;
    if (adv && !skip) N1 = make_int4(Cn, (int32_t)e2t, (int32_t)e2c, seen_term);

    // 5. sticky flags, the step of the first one
    const uint32_t was = (uint32_t)H0.x, now = was | group_or(bits);
    const bool head = live && r == 0;
    const bool newly = was == 0 && now != 0;
    const int4 N0 = make_int4((int32_t)now, newly ? step : H0.y, lead_term, lead_rep);
    if (head && differ(N0, H0)) hdr[2 * g] = N0;
    if (head && differ(N1, H1)) hdr[2 * g + 1] = N1;

    const uint32_t got = head ? now & ~was : 0u;
    const unsigned long long b_new = __ballot(head && newly), b_fl = __ballot(head && now != 0),
                             b_t = __ballot(got & RAFT_AUDIT_TERM_REGRESSED), b_v = __ballot(got & RAFT_AUDIT_VOTE_CHANGED),
                             b_2 = __ballot(got & RAFT_AUDIT_TWO_LEADERS), b_c = __ballot(got & RAFT_AUDIT_COMMIT_CHANGED),
                             b_l = __ballot(got & RAFT_AUDIT_LEADER_INCOMPLETE);
    const uint32_t unk = (uint32_t)(__popcll(__ballot(unk_a)) + __popcll(__ballot(unk_b)) + __popcll(__ballot(unk_n)));
    if ((threadIdx.x & 63) == 0) {
        unsigned long long* line = stripe_of(cnt, wave_index());
        tally_ballot(line, AW_NEWLY, b_new);
        tally_ballot(line, AW_FLAGGED, b_fl);
        tally_ballot(line, AW_TERM, b_t);
        tally_ballot(line, AW_VOTE, b_v);
        tally_ballot(line, AW_TWO, b_2);
        tally_ballot(line, AW_COMMIT, b_c);
        tally_ballot(line, AW_LEADER, b_l);
        tally(line, AW_UNKNOWN, unk);
    }
}

// the report's source (raft_stream.h): a group's first header quad, a record iff its flags are set
struct AuditSource {
    using Word = uint4;
    static constexpr int WORDS = 1, TALLIES = 1;                        // word 0 (AW_NEWLY's place): the flagged groups
    struct Item {
        int4 H0;
        bool hit;
    };
    const int4* __restrict__ hdr;

    __device__ __forceinline__ Item eval(int64_t g, bool live) const {
        const int4 H0 = hdr[2 * g];
        return Item{H0, live && H0.x != 0};
    }
    __device__ __forceinline__ void tallies(const Item& it, bool, unsigned long long (&b)[TALLIES]) const {
        b[0] = __ballot(it.hit);
    }
    __device__ __forceinline__ void record(const Item& it, int64_t g, uint4* st) const {
        st[0] = make_uint4((uint32_t)((uint64_t)g & 0xFFFFFFFFu), (uint32_t)((uint64_t)g >> 32), (uint32_t)it.H0.x,
                           (uint32_t)it.H0.y);
    }
    __device__ __forceinline__ void commit(const Item&, int64_t) const {}   // a report changes nothing
    static int64_t total(const unsigned long long* w) { return (int64_t)w[0]; }
};

// the zero state of groups [g0, g0 + n), enqueued on the engine stream
int fill(raft_audit* a, int64_t g0, int64_t n) {
    const int R = a->e->p.R;
    audit_fill_kernel<<<grid_of(n * R), BLOCK, 0, a->e->stream>>>(a->hdr, a->pairs, g0, n, R);
    HIP_TRY(hipGetLastError());
    return RAFT_OK;
}

int report(raft_audit* a, int64_t g0, int64_t n, raft_audit_event* out, int64_t max_events,
           raft_audit_report_info* info, bool out_on_host) {
    return ledger_report<AuditSource>(a, "null audit", g0, n, out, max_events, out_on_host, info, [&](AuditSource& s) {
        s.hdr = a->hdr;
        return RAFT_OK;
    });
}

}  // namespace

extern "C" {

int raft_audit_create(raft_engine* e, raft_audit** out) {
    if (int rc = create_args(e, out)) return rc;
    const size_t hdr_b = al256((size_t)e->p.G * 32), pair_b = al256((size_t)e->dp.GR * 8);
    return ledger_create(e, out, hdr_b + pair_b, "the audit's ledger", [&](raft_audit* a) {
        a->hdr = (int4*)a->mem;
        a->pairs = (int2*)(a->mem + hdr_b);
        return raft_audit_reset(a);
    });
}

int raft_audit_destroy(raft_audit* a) { return ledger_destroy(a); }

int raft_audit_reset(raft_audit* a) {
    return ledger_reset(a, "null audit", [&](raft_engine* e) {
        e->fork_needed = true;
        return fill(a, 0, e->p.G);
    });
}

int64_t raft_audit_device_bytes(raft_audit* a) { return ledger_bytes(a); }

int raft_audit_observe(raft_audit* a, int64_t g0, int64_t n, raft_audit_info* info) {
    Counts c{};
    if (int rc = ledger_observe(a, "null audit", g0, n, info, c, [&](unsigned grid, unsigned long long* cnt) {
            audit_observe_kernel<<<grid, BLOCK, 0, a->e->stream>>>(a->e->dp, a->hdr, a->pairs, g0, n,
                                                                   (int32_t)(uint32_t)a->e->t, cnt);
        }))
        return rc;
    info->newly_flagged = (int64_t)c.w[AW_NEWLY];
    info->flagged = (int64_t)c.w[AW_FLAGGED];
    info->term_regressed = (int64_t)c.w[AW_TERM];
    info->vote_changed = (int64_t)c.w[AW_VOTE];
    info->two_leaders = (int64_t)c.w[AW_TWO];
    info->commit_changed = (int64_t)c.w[AW_COMMIT];
    info->leader_incomplete = (int64_t)c.w[AW_LEADER];
    info->unknown = (int64_t)c.w[AW_UNKNOWN];
    return RAFT_OK;
}

int raft_audit_report(raft_audit* a, int64_t g0, int64_t n, raft_audit_event* out_host, int64_t max_events,
                      raft_audit_report_info* info) {
    return report(a, g0, n, out_host, max_events, info, true);
}

int raft_audit_report_dev(raft_audit* a, int64_t g0, int64_t n, raft_audit_event* out_dev, int64_t max_events,
                          raft_audit_report_info* info) {
    return report(a, g0, n, out_dev, max_events, info, false);
}

// the exported row of a group is its two header quads, then its R pairs: two regions on the device
int raft_audit_read(raft_audit* a, int64_t g0, int64_t n, int32_t* out) {
    return table_call(check_ledger(a, g0, n, "null audit"), n, out, [&]() -> int {
        const int R = a->e->p.R, W = 8 + 2 * R;
        std::vector<int32_t> h((size_t)n * 8), pr((size_t)n * R * 2);
        if (int rc = rows_out(a->e, {{a->hdr + 2 * g0, h.data(), h.size() * 4}, {a->pairs + g0 * R, pr.data(), pr.size() * 4}}))
            return rc;
        for (int64_t k = 0; k < n; ++k) {
            std::memcpy(out + k * W, h.data() + k * 8, 32);
            std::memcpy(out + k * W + 8, pr.data() + k * R * 2, (size_t)R * 8);
        }
        return RAFT_OK;
    });
}

int raft_audit_write(raft_audit* a, int64_t g0, int64_t n, const int32_t* in) {
    return table_call(check_ledger(a, g0, n, "null audit"), n, in, [&]() -> int {
        raft_engine* e = a->e;
        const int R = e->p.R, W = 8 + 2 * R;
        for (int64_t k = 0; k < n; ++k) {
            const int32_t* w = in + k * W;
            if ((uint32_t)w[0] & ~AUDIT_ALL) return raft_internal_fail(RAFT_EINVAL, "a ledger's flags hold unknown bits");
            if (w[3] < -1 || w[3] >= R) return raft_internal_fail(RAFT_EINVAL, "a ledger's lead_replica must be in -1..R-1");
            if (w[4] < 0 || w[4] > e->p.log_cap)
                return raft_internal_fail(RAFT_EINVAL, "a ledger's anchor_count must be in 0..log_cap");
        }
        std::vector<int32_t> h((size_t)n * 8), pr((size_t)n * R * 2);
        for (int64_t k = 0; k < n; ++k) {
            std::memcpy(h.data() + k * 8, in + k * W, 32);
            std::memcpy(pr.data() + k * R * 2, in + k * W + 8, (size_t)R * 8);
        }
        e->fork_needed = true;
        return rows_in(e, {{a->hdr + 2 * g0, h.data(), h.size() * 4}, {a->pairs + g0 * R, pr.data(), pr.size() * 4}});
    });
}

}  // extern "C"
