// raft_nemesis.hip — scripted network faults (include/raft_engine.h
// raft_isolate_batch*, raft_engine_heal_network*, raft_engine_list_isolated*):
// the group's isolation word (gx[GX_ISO], rem << 8 | replica; raft_step.h phase
// H and lost_net) aimed by the caller instead of drawn by the churn harness.
// A side path between two step launches: the only state word written is that
// one, the step kernel does the rest under its own rules.
//
// Kernels of its own, on the plumbing of raft_engine_impl.h and raft_stream.h:
//   clear     one thread per message: its group against the engine (a group
//             outside fails the batch before a word or a ticket is written),
//             and ~0 into the group's word of a per-batch claim table (engine
//             staging, one word per group): only the words the batch names
//             are cleared, so a small batch costs O(n), not O(G).
//   claim     one thread per message: target and steps against their ranges,
//             and for a message that passes an atomicMin of its batch position
//             into the group's claim word.  A minimum does not depend on the
//             order of its operands, so the winner is the lowest position
//             whatever the schedule.
//   isolate   one thread per message: an out-of-range message answers INVALID
//             and reads nothing more; a message whose position is not the
//             group's claim answers DUPLICATE with the claim; the winner reads
//             the isolation word and, for a leader selector, the R role / term
//             words (find_newest_leader / find_leader), and stores at most one
//             4-byte word.  One 16-byte ticket store each.  Only a group's
//             winner reads or writes the group's word: no thread reads a word
//             another thread writes.
//   heal      one thread per group: the mask byte and the isolation word; at
//             most one 4-byte store (zero, what phase H's expiry leaves); the
//             counts per wave (ballot and popcount), one atomic per nonzero
//             word into the wave's stripe.
//   list      raft_stream.h's flag / scan / write over a source object: the
//             isolation word, and for a running one quad 0 of the isolated
//             replica (its role); read-only.
#include <hip/hip_runtime.h>

#include <string>

#include "raft_ledger.h"

using namespace raft;

namespace {

static_assert(sizeof(raft_isolate_ticket) == 16 && sizeof(raft_isolated) == 16 && sizeof(raft_heal_info) == 32 &&
                  sizeof(raft_isolated_info) == 32, "record layouts of the C-ABI");

constexpr int32_t MAX_STEPS = RAFT_ISOLATE_MAX_STEPS;                  // restart's MAX_DOWN_STEPS: rem << 8 stays positive

// the status words of an isolate, striped as a transfer's (DevWords, raft_engine_impl.h), at the head of cli; the
// claim table [G] follows them
enum { NW_RANGE = 0, NW_SET = 1, NW_WORDS = 2, NW_LINE = 16, NW_STRIPES = 64 };
using Status = DevWords<unsigned int, NW_STRIPES, NW_LINE, NW_WORDS, false>;
// the counts of a heal, striped as a restart's totals, at the head of aux
enum { HL_HEALED = 0, HL_IDLE = 1, HL_KEPT = 2, HL_WORDS = 3 };
using Counts = DevWords<unsigned long long, HDR_STRIPES, HDR_LINE, HL_WORDS, true>;

// OR 1 into status word `w` of the wave's stripe, once per wave: every lane of
// the wave calls this.  The range word stays in stripe 0, where the isolate
// pass reads it.
__device__ __forceinline__ void wave_flag(unsigned int* flags, int w, bool mine) {
    const unsigned long long any = __ballot(mine);
    const unsigned stripe = w == NW_RANGE ? 0u : (blockIdx.x * WAVES_PER_BLOCK + (threadIdx.x >> 6)) & (NW_STRIPES - 1);
    if ((threadIdx.x & 63) == 0 && any) atomicOr(&flags[stripe * NW_LINE + w], 1u);
}

// steps left of an isolation word, 0 if it is not running (rem << 8 | replica, raft_step.h phase H)
__device__ __forceinline__ int32_t running(int32_t iso) { return max(iso >> 8, 0); }

__device__ __forceinline__ bool in_range(int32_t want, int32_t steps, int R) {
    return want >= RAFT_ISOLATE_LOWEST_LEADER && want < R && steps >= 1 && steps <= MAX_STEPS;
}

__global__ __launch_bounds__(BLOCK) void isolate_clear_kernel(const int64_t* __restrict__ group, int n, int64_t G,
                                                              uint32_t* __restrict__ claim, unsigned int* flags) {
    const int64_t m = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const bool live = m < n;
    const int64_t g = group[live ? m : n - 1];
    const bool inside = g >= 0 && g < G;
    // unclaimed: above every batch position (n < 2^31).  0 <= g < G: inside the table; every writer stores the same
    if (live && inside) claim[g] = 0xFFFFFFFFu;
    wave_flag(flags, NW_RANGE, live && !inside);
}

__global__ __launch_bounds__(BLOCK) void isolate_claim_kernel(const int64_t* __restrict__ group,
                                                              const int32_t* __restrict__ target,
                                                              const int32_t* __restrict__ steps, int n, int64_t G, int R,
                                                              uint32_t* __restrict__ claim) {
    const int64_t m = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (m >= n) return;
    const int64_t g = group[m];
    if (g >= 0 && g < G && in_range(target[m], steps[m], R)) atomicMin(&claim[g], (uint32_t)m);   // 0 <= g < G: inside the table
}

__global__ __launch_bounds__(BLOCK) void isolate_kernel(DevParams p, const int64_t* __restrict__ group,
                                                        const int32_t* __restrict__ target,
                                                        const int32_t* __restrict__ steps, int32_t flags_arg,
                                                        const uint32_t* __restrict__ claim, int4* __restrict__ ticket,
                                                        int n, unsigned int* flags) {
    if (*(volatile unsigned int*)&flags[NW_RANGE]) return;             // a group outside the engine: nothing is written
    const int64_t m = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const bool live = m < n;
    const int64_t mm = live ? m : n - 1;
    const int64_t g = group[mm];                                        // (the range word was clear: every group is inside)
    const int32_t want = target[mm], st = steps[mm];
    const int R = p.R;
    bool set = false;
    if (live) {
        int4 tk = make_int4(-1, st, RAFT_ISOLATE_INVALID, 0);           // raft_isolate_ticket: replica, steps, status, prev
        if (g >= 0 && g < p.G && in_range(want, st, R)) {
            const uint32_t won = claim[g];
            if (won != (uint32_t)m) {
                tk = make_int4(-1, st, RAFT_ISOLATE_DUPLICATE, (int32_t)won);
            } else {
                int32_t* word = &p.gx[GX_ISO * p.G + g];
                const int32_t iso = *word;
                int32_t rep = want;
                if (want < 0) rep = (want == RAFT_ISOLATE_NEWEST_LEADER ? find_newest_leader(p, g) : find_leader(p, g)).r;
                if (rep < 0) {
                    tk = make_int4(-1, st, RAFT_ISOLATE_NO_LEADER, iso);
                } else if (running(iso) > 0 && !(flags_arg & RAFT_ISOLATE_REPLACE)) {
                    tk = make_int4(rep, st, RAFT_ISOLATE_BUSY, iso);
                } else {
                    *word = st << 8 | rep;                              // 0 <= rep < R <= 8, 1 <= st < 2^23
                    tk = make_int4(rep, st, RAFT_ISOLATE_SET, iso);
                    set = true;
                }
            }
        }
        ticket[m] = tk;
    }
    wave_flag(flags, NW_SET, set);
}

__global__ __launch_bounds__(BLOCK) void heal_kernel(DevParams p, int64_t g0, int64_t n, const uint8_t* __restrict__ mask,
                                                     unsigned long long* hdr) {
    const int64_t j = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const bool live = j < n;
    const int64_t jj = live ? j : n - 1;
    const int64_t g = g0 + jj;                                          // g0 <= g < g0 + n <= G (check_groups)
    const uint32_t mk = mask ? mask[jj] : 0u;
    int32_t* word = &p.gx[GX_ISO * p.G + g];
    const int32_t iso = *word;
    const int32_t rep = iso & 0xFF;
    const bool run = live && running(iso) > 0;
    const bool heal = run && (!mask || (rep < 8 && ((mk >> rep) & 1u)));   // no mask: any replica
    if (heal) *word = 0;                                                // as phase H leaves an expired word: all of it zero
    const unsigned long long b_heal = __ballot(heal), b_idle = __ballot(live && !run), b_kept = __ballot(run && !heal);
    if ((threadIdx.x & 63) == 0 && live) {                              // lane 0 live: the wave is inside the range
        unsigned long long* line = stripe_of(hdr, wave_index());
        tally_ballot(line, HL_HEALED, b_heal);
        tally_ballot(line, HL_IDLE, b_idle);
        tally_ballot(line, HL_KEPT, b_kept);
    }
}

// the listing's source (raft_stream.h): a group whose isolation word is running
struct IsolatedSource {
    using Word = uint4;
    static constexpr int WORDS = 1, TALLIES = 1;
    struct Item {
        int32_t iso;
        bool hit;
    };
    DevParams p;

    __device__ __forceinline__ Item eval(int64_t g, bool live) const {
        const int32_t iso = p.gx[GX_ISO * p.G + g];
        return Item{iso, live && running(iso) > 0};
    }
    __device__ __forceinline__ void tallies(const Item& it, bool, unsigned long long (&b)[TALLIES]) const {
        b[0] = __ballot(it.hit);
    }
    __device__ __forceinline__ void record(const Item& it, int64_t g, uint4* st) const {
        const int32_t rep = it.iso & 0xFF;
        // the replica's role now; a word whose replica is outside the group (only write_state could leave one) reads
        // replica R - 1's quad and reports no role
        const int32_t role = quad(p, 0, g * p.R + min(rep, p.R - 1))->z;
        const uint32_t rr = (uint32_t)(rep & 0xFFFF) | (uint32_t)((rep < p.R ? role : -1) & 0xFFFF) << 16;
        st[0] = make_uint4((uint32_t)((uint64_t)g & 0xFFFFFFFFu), (uint32_t)((uint64_t)g >> 32), rr, (uint32_t)(it.iso >> 8));
    }
    __device__ __forceinline__ void commit(const Item&, int64_t) const {}   // read-only
    static int64_t total(const unsigned long long* w) { return (int64_t)w[0]; }
};

int isolate_dev(raft_engine* e, const int64_t* group, const int32_t* target, const int32_t* steps, int32_t flags,
                raft_isolate_ticket* ticket, int n) {
    e->fork_needed = true;                          // later step launches wait for the words set here
    // staging: the status words, then the claim table, one word per group of the engine
    const size_t table = (size_t)e->p.G * sizeof(uint32_t);
    if (int rc = raft_internal_grow_dev(e, &e->cli, &e->cli_bytes, Status::BYTES + table)) return rc;
    Status st;
    if (int rc = st.zero(e, e->cli)) return rc;
    uint32_t* claim = (uint32_t*)(e->cli + Status::BYTES);
    const unsigned grid = grid_of(n);
    isolate_clear_kernel<<<grid, BLOCK, 0, e->stream>>>(group, n, e->p.G, claim, st.dev);
    isolate_claim_kernel<<<grid, BLOCK, 0, e->stream>>>(group, target, steps, n, e->p.G, e->p.R, claim);
    isolate_kernel<<<grid, BLOCK, 0, e->stream>>>(e->dp, group, target, steps, flags, claim, (int4*)ticket, n, st.dev);
    HIP_TRY(hipGetLastError());
    if (int rc = st.fetch(e)) return rc;
    if (st.w[NW_RANGE])
        return raft_internal_fail(RAFT_ERANGE, "an isolation's group is outside the engine; nothing was written");
    if (st.w[NW_SET]) e->iso_written = true;        // an isolation word: NET_ISO kernels from now on
    return RAFT_OK;
}

int check_isolate(raft_engine* e, int64_t n, int32_t flags, bool any_null) {
    if (int rc = check_args(e, n, any_null)) return rc;
    if (flags & ~RAFT_ISOLATE_REPLACE) return raft_internal_fail(RAFT_EINVAL, "unknown isolate flag bits");
    return RAFT_OK;
}

int heal(raft_engine* e, int64_t g0, int64_t n, bool host, const uint8_t* mask, raft_heal_info* info) {
    if (!e) return raft_internal_fail(RAFT_EINVAL, "null engine");
    if (!info) return raft_internal_fail(RAFT_EINVAL, "null info");
    *info = raft_heal_info{};
    if (int rc = check_groups(e, g0, n)) return rc;
    if (n == 0) return RAFT_OK;
    HIP_TRY(hipSetDevice(e->device));
    e->fork_needed = true;                           // later step launches wait for the words cleared here
    host = host && mask;
    // staging: the counts, then the device copy of a host mask
    if (int rc = raft_internal_grow_dev(e, &e->aux, &e->aux_bytes, Counts::BYTES + (host ? (size_t)n : 0))) return rc;
    Counts c;
    if (int rc = c.zero(e, e->aux)) return rc;
    if (host) {
        HIP_TRY(hipMemcpyAsync(e->aux + Counts::BYTES, mask, (size_t)n, hipMemcpyHostToDevice, e->stream));
        mask = (const uint8_t*)(e->aux + Counts::BYTES);
    }
    heal_kernel<<<grid_of(n), BLOCK, 0, e->stream>>>(e->dp, g0, n, mask, c.dev);
    HIP_TRY(hipGetLastError());
    if (int rc = c.fetch(e)) return rc;
    info->healed = (int64_t)c.w[HL_HEALED];
    info->idle = (int64_t)c.w[HL_IDLE];
    info->kept = (int64_t)c.w[HL_KEPT];
    return RAFT_OK;
}

int list(raft_engine* e, int64_t g0, int64_t n, raft_isolated* out, int64_t max_events, raft_isolated_info* info,
         bool out_on_host) {
    if (!e) return raft_internal_fail(RAFT_EINVAL, "null engine");
    return list_records<IsolatedSource>(e, g0, n, out, max_events, out_on_host, info, &raft_isolated_info::running,
                                        [&](IsolatedSource& s) {
                                            s.p = e->dp;
                                            return RAFT_OK;
                                        });
}

}  // namespace

extern "C" {

int raft_isolate_batch_dev(raft_engine* e, const int64_t* group, const int32_t* target, const int32_t* steps,
                           int32_t flags, raft_isolate_ticket* ticket, int64_t n) {
    if (int rc = check_isolate(e, n, flags, !group || !target || !steps || !ticket)) return rc;
    if (n == 0) return RAFT_OK;
    if (!aligned16(ticket)) return raft_internal_fail(RAFT_EINVAL, "the ticket buffer must be 16-byte aligned");
    HIP_TRY(hipSetDevice(e->device));
    return isolate_dev(e, group, target, steps, flags, ticket, (int)n);
}

int raft_isolate_batch(raft_engine* e, const int64_t* group, const int32_t* target, const int32_t* steps, int32_t flags,
                       raft_isolate_ticket* ticket, int64_t n) {
    if (int rc = check_isolate(e, n, flags, !group || !target || !steps || !ticket)) return rc;
    if (n == 0) return RAFT_OK;
    HIP_TRY(hipSetDevice(e->device));
    const void* src[3] = {group, target, steps};
    const size_t bytes[3] = {(size_t)n * 8, (size_t)n * 4, (size_t)n * 4};
    Staged s;
    if (int rc = stage_in(e, src, bytes, 3, (size_t)n * sizeof(raft_isolate_ticket), s)) return rc;
    if (int rc = isolate_dev(e, (const int64_t*)(e->cio + s.off[0]), (const int32_t*)(e->cio + s.off[1]),
                             (const int32_t*)(e->cio + s.off[2]), flags, (raft_isolate_ticket*)(e->cio + s.out_off), (int)n))
        return rc;                                                      // RAFT_ERANGE: no ticket was written
    return stage_out(e, s, ticket);
}

int raft_engine_heal_network(raft_engine* e, int64_t g0, int64_t n, const uint8_t* mask_host, raft_heal_info* info) {
    return heal(e, g0, n, true, mask_host, info);
}

int raft_engine_heal_network_dev(raft_engine* e, int64_t g0, int64_t n, const uint8_t* mask_dev, raft_heal_info* info) {
    return heal(e, g0, n, false, mask_dev, info);
}

int raft_engine_list_isolated(raft_engine* e, int64_t g0, int64_t n, raft_isolated* out_host, int64_t max_events,
                              raft_isolated_info* info) {
    return list(e, g0, n, out_host, max_events, info, true);
}

int raft_engine_list_isolated_dev(raft_engine* e, int64_t g0, int64_t n, raft_isolated* out_dev, int64_t max_events,
                                  raft_isolated_info* info) {
    return list(e, g0, n, out_dev, max_events, info, false);
}

}  // extern "C"
