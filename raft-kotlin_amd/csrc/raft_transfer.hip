// raft_transfer.hip — leadership transfer (include/raft_engine.h
// raft_transfer_batch*, raft_engine_resolve_transfers*, raft_engine_evacuate*):
// Raft's TimeoutNow (Ongaro's thesis §3.10) as a side path between two step
// launches.  A transfer is "the target's election timer fires now": the only
// word written is the target's electionMs = 1, and phase T of the next step
// does the rest under the step kernel's own rules.
//
// Kernels of its own, on the plumbing of raft_engine_impl.h:
//   range     one thread per message: its group against the engine (transfer
//             only: a group outside the engine fails the batch before a word or
//             a ticket is written)
//   transfer  one thread per message: the R role / term / flags words (quad 0 of
//             each replica), lastIndex and the cached tail term (quad 1) of the
//             target -- of all R replicas for RAFT_TRANSFER_AUTO -- issued with
//             them, the group's isolation word, and quad 1 of the leader once
//             quad 0 has named it; at most one 4-byte store (the target's
//             electionMs) and one 16-byte ticket store.  electionMs itself is
//             never loaded: no thread reads a word another thread writes.
//   resolve   one thread per message: the R quad-0 words; one 16-byte store
//   evacuate  one thread per group: the mask byte, the R quad-0 words, and for
//             groups led from inside the mask quad 1 of the R replicas and the
//             isolation word; the counts are reduced per wave (ballot and
//             popcount) before one atomic per nonzero word into the wave's stripe.
#include <hip/hip_runtime.h>

#include <string>

#include "raft_stream.h"

using namespace raft;

namespace {

static_assert(sizeof(raft_transfer_ticket) == 16 && sizeof(raft_transfer_state) == 16 &&
                  sizeof(raft_evacuate_info) == 64, "record layouts of the C-ABI");

// the status words of a batch call, striped as raft_read.hip's (DevWords, raft_engine_impl.h), at the head of cli
enum { TW_RANGE = 0, TW_INVAL = 1, TW_WORDS = 2, TW_LINE = 16, TW_STRIPES = 64 };
using Status = DevWords<unsigned int, TW_STRIPES, TW_LINE, TW_WORDS, false>;
// the counts of an evacuate, striped as a restart's totals, at the head of aux
enum { EV_LED = 0, EV_SENT = 1, EV_NO_TARGET = 2, EV_BEHIND = 3, EV_BUSY = 4, EV_WORDS = 5 };
using Counts = DevWords<unsigned long long, HDR_STRIPES, HDR_LINE, EV_WORDS, true>;

// OR 1 into status word `w` of the wave's stripe, once per wave: every lane of
// the wave calls this.  The range word stays in stripe 0, where the transfer
// pass reads it.
__device__ __forceinline__ void wave_flag(unsigned int* flags, int w, bool mine) {
    const unsigned long long any = __ballot(mine);
    const unsigned stripe = w == TW_RANGE ? 0u : (blockIdx.x * WAVES_PER_BLOCK + (threadIdx.x >> 6)) & (TW_STRIPES - 1);
    if ((threadIdx.x & 63) == 0 && any) atomicOr(&flags[stripe * TW_LINE + w], 1u);
}

// lastIndex and the cached tail term of a replica (words 0 and 2 of quad 1),
// without its electionMs (word 3, the word a transfer writes)
struct Tail {
    int32_t last, term;
};
__device__ __forceinline__ Tail load_tail(const DevParams& p, int64_t idx) {
    const int32_t* q = (const int32_t*)quad(p, 1, idx);
    return Tail{q[0], q[2]};
}

// the replica the isolation word cuts off in the next step, -1 if none (rem << 8 | replica, raft_step.h phase H)
__device__ __forceinline__ int32_t isolated(int32_t iso) { return (iso >> 8) > 0 ? (iso & 0xFF) : -1; }

// Why replica r cannot take over from a leader whose tail is `lead`:
// RAFT_TRANSFER_SENT if it can, else BEHIND, BUSY or UNREACHABLE, in that order.
__device__ __forceinline__ int32_t judge(const int4& q0, const Tail& t, const Tail& lead, int r, int32_t iso_rep) {
    if (t.last != lead.last || t.term != lead.term) return RAFT_TRANSFER_BEHIND;
    const uint32_t fl = (uint32_t)q0.w;
    if (q0.z != RAFT_FOLLOWER || !(fl & FL_ARMED) || (fl & (FL_ELECTING | FL_BACKOFF | FL_PRST))) return RAFT_TRANSFER_BUSY;
    if (r == iso_rep) return RAFT_TRANSFER_UNREACHABLE;
    return RAFT_TRANSFER_SENT;
}

// the newest leader among loaded role words (find_newest_leader's rule, raft_engine_impl.h)
__device__ __forceinline__ Lead newest_of(const int4 (&q)[RAFT_MAX_R], int R) {
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

// element r (0 <= r < RAFT_MAX_R) of an array held in registers: a select chain, not a dynamic index
template <class T>
__device__ __forceinline__ T pick(const T (&a)[RAFT_MAX_R], int r) {
    T v = a[0];
#pragma unroll
    for (int s = 1; s < RAFT_MAX_R; ++s) v = s == r ? a[s] : v;
    return v;
}

// AUTO's choice: the first replica after `from`, cyclically, that is not in
// `excluded` and that judge() lets through; -1 if none.  seen: bit s of it is
// set when some candidate was refused with status s.
__device__ __forceinline__ int32_t choose(const int4 (&q0)[RAFT_MAX_R], const Tail (&t)[RAFT_MAX_R], int R, int from,
                                          uint32_t excluded, int32_t iso_rep, uint32_t& seen) {
    const Tail lead = pick(t, from);
    int32_t to = -1, nearest = RAFT_MAX_R;
    seen = 0;
#pragma unroll
    for (int r = 0; r < RAFT_MAX_R; ++r) {
        if (r < R && r != from && !((excluded >> r) & 1u)) {
            const int32_t st = judge(q0[r], t[r], lead, r, iso_rep);
            const int32_t k = r - from + (r < from ? R : 0);            // its place after `from`, cyclically: 1..R-1
            if (st != RAFT_TRANSFER_SENT) {
                seen |= 1u << st;
            } else if (k < nearest) {
                nearest = k;
                to = r;
            }
        }
    }
    return to;
}

__global__ __launch_bounds__(BLOCK) void transfer_range_kernel(const int64_t* __restrict__ group, int n, int64_t G,
                                                               unsigned int* flags) {
    const int m = blockIdx.x * BLOCK + threadIdx.x;
    const bool live = m < n;
    const int64_t g = group[live ? m : n - 1];
    wave_flag(flags, TW_RANGE, live && (g < 0 || g >= G));
}

__global__ __launch_bounds__(BLOCK) void transfer_kernel(DevParams p, const int64_t* __restrict__ group,
                                                         const int32_t* __restrict__ target,
                                                         int4* __restrict__ ticket, int n, unsigned int* flags) {
    if (*(volatile unsigned int*)&flags[TW_RANGE]) return;             // a group outside the engine: nothing is written
    const int m = blockIdx.x * BLOCK + threadIdx.x;
    if (m >= n) return;
    const int64_t g = group[m];
    const int32_t want = target[m];
    const int R = p.R;
    int4 tk = make_int4(-1, 0, -1, RAFT_TRANSFER_INVALID);              // raft_transfer_ticket: from, term, target, status
    if (g >= 0 && g < p.G && want >= RAFT_TRANSFER_AUTO && want < R) {  // (the range word was clear: every group is inside)
        // every load that does not depend on the leader's id, in flight at once
        int4 q0[RAFT_MAX_R];
        load_roles(p, g, q0);
        const int32_t iso_rep = isolated(p.gx[GX_ISO * p.G + g]);
        Tail t[RAFT_MAX_R];                                             // AUTO: every replica's
#pragma unroll
        for (int r = 0; r < RAFT_MAX_R; ++r) t[r] = want < 0 ? load_tail(p, g * R + min(r, R - 1)) : Tail{0, 0};
        // a named target's words, through addresses of their own (its quad 0 is in the sector load_roles
        // reads): the arrays stay in registers, indexed by constants only
        const int64_t tidx = g * R + max(want, 0);
        const int4 tq0 = *quad(p, 0, tidx);
        const Tail tt = load_tail(p, tidx);
        const Lead l = newest_of(q0, R);
        tk = make_int4(-1, 0, -1, RAFT_TRANSFER_NO_LEADER);
        if (l.r >= 0) {
            int32_t to = -1, st;
            if (want == l.r) {
                st = RAFT_TRANSFER_SELF;
            } else if (want >= 0) {
                const Tail lead = load_tail(p, g * R + l.r);
                st = judge(tq0, tt, lead, want, iso_rep);
                to = want;
            } else {
                uint32_t seen;
                to = choose(q0, t, R, l.r, 0u, iso_rep, seen);
                st = to >= 0 ? RAFT_TRANSFER_SENT : RAFT_TRANSFER_NO_TARGET;
            }
            if (st == RAFT_TRANSFER_SENT)                               // 0 <= to < R: replica g * R + to is inside the state
                ((int32_t*)quad(p, 1, g * R + to))[3] = 1;              // electionMs: phase T of the next step fires it
            tk = make_int4(l.r, l.term, st == RAFT_TRANSFER_SENT ? to : -1, st);
        }
    }
    ticket[m] = tk;
}

__global__ __launch_bounds__(BLOCK) void transfer_resolve_kernel(DevParams p, const int64_t* __restrict__ group,
                                                                 const int4* __restrict__ ticket, int4* __restrict__ out,
                                                                 int n, unsigned int* flags) {
    const int m = blockIdx.x * BLOCK + threadIdx.x;
    const bool live = m < n;
    const int mm = live ? m : n - 1;
    const int64_t g = group[mm];
    const int4 tk = ticket[mm];                                         // (from, term, target, status)
    const int R = p.R;
    const bool g_ok = g >= 0 && g < p.G;
    const bool sent = tk.w == RAFT_TRANSFER_SENT;
    const bool t_ok = !sent || (tk.x >= 0 && tk.x < R && tk.z >= 0 && tk.z < R);
    int4 rec = make_int4(RAFT_TRANSFER_INVALID, -1, 0, 0);              // raft_transfer_state: status, leader, term, reserved
    if (live && g_ok && t_ok) {
        if (!sent) {
            rec.x = RAFT_TRANSFER_NONE;
        } else {
            int4 q[RAFT_MAX_R];
            load_roles(p, g, q);
            // the newest LEADER above the ticket's term, and whether the target is one
            int32_t best = -1, bterm = 0, tterm = 0;
            bool target_leads = false;
#pragma unroll
            for (int r = RAFT_MAX_R - 1; r >= 0; --r) {
                if (r < R && q[r].z == RAFT_LEADER && q[r].x > tk.y) {
                    if (best < 0 || q[r].x >= bterm) {
                        best = r;
                        bterm = q[r].x;
                    }
                    if (r == tk.z) {
                        target_leads = true;
                        tterm = q[r].x;
                    }
                }
            }
            if (target_leads) rec = make_int4(RAFT_TRANSFER_COMPLETED, tk.z, tterm, 0);
            else if (best >= 0) rec = make_int4(RAFT_TRANSFER_SUPERSEDED, best, bterm, 0);
            else rec = make_int4(RAFT_TRANSFER_PENDING, -1, 0, 0);
        }
    }
    if (live) out[m] = rec;
    wave_flag(flags, TW_RANGE, live && !g_ok);
    wave_flag(flags, TW_INVAL, live && g_ok && !t_ok);
}

__global__ __launch_bounds__(BLOCK) void evacuate_kernel(DevParams p, int64_t g0, int64_t n,
                                                         const uint8_t* __restrict__ mask, unsigned long long* hdr) {
    const int64_t j = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const bool live = j < n;
    const int64_t g = g0 + (live ? j : n - 1);                          // g0 <= g < g0 + n <= G (check_groups)
    const int R = p.R;
    const uint32_t mk = mask[live ? j : n - 1] & ((1u << R) - 1u);      // bits at or above R are ignored
    int4 q0[RAFT_MAX_R];
    load_roles(p, g, q0);
    const Lead l = newest_of(q0, R);
    const bool led = live && l.r >= 0 && ((mk >> l.r) & 1u);
    bool sent = false, behind = false, busy = false;
    if (led) {
        const int32_t iso_rep = isolated(p.gx[GX_ISO * p.G + g]);
        Tail t[RAFT_MAX_R];
#pragma unroll
        for (int r = 0; r < RAFT_MAX_R; ++r) t[r] = load_tail(p, g * R + min(r, R - 1));
        uint32_t seen;
        const int32_t to = choose(q0, t, R, l.r, mk, iso_rep, seen);
        if (to >= 0) {
            sent = true;
            ((int32_t*)quad(p, 1, g * R + to))[3] = 1;                  // 0 <= to < R
        } else {
            behind = (seen >> RAFT_TRANSFER_BEHIND) & 1u;
            busy = ((seen >> RAFT_TRANSFER_BUSY) | (seen >> RAFT_TRANSFER_UNREACHABLE)) & 1u;
        }
    }
    // the counts: one atomic per nonzero word and wave
    const unsigned long long b_led = __ballot(led), b_sent = __ballot(sent), b_behind = __ballot(behind),
                             b_busy = __ballot(busy);
    if ((threadIdx.x & 63) == 0 && b_led) {
        unsigned long long* line = stripe_of(hdr, wave_index());
        const unsigned long long n_led = __popcll(b_led), n_sent = __popcll(b_sent);
        atomicAdd(line + EV_LED, n_led);                                // (b_led != 0)
        tally(line, EV_SENT, n_sent);
        tally(line, EV_NO_TARGET, n_led - n_sent);
        tally_ballot(line, EV_BEHIND, b_behind);
        tally_ballot(line, EV_BUSY, b_busy);
    }
}

int zeroed_status(raft_engine* e, Status& st) {
    if (int rc = raft_internal_grow_dev(e, &e->cli, &e->cli_bytes, Status::BYTES)) return rc;
    return st.zero(e, e->cli);
}

int transfer_dev(raft_engine* e, const int64_t* group, const int32_t* target, raft_transfer_ticket* ticket, int n) {
    e->fork_needed = true;                          // later step launches wait for the timers set here
    raft_internal_ensure_cache(e);                  // the cached tail term is compared: rebuilt first if a host write left it stale
    Status st;
    if (int rc = zeroed_status(e, st)) return rc;
    const unsigned grid = (unsigned)((n + BLOCK - 1) / BLOCK);
    transfer_range_kernel<<<grid, BLOCK, 0, e->stream>>>(group, n, e->p.G, st.dev);
    transfer_kernel<<<grid, BLOCK, 0, e->stream>>>(e->dp, group, target, (int4*)ticket, n, st.dev);
    HIP_TRY(hipGetLastError());
    if (int rc = st.fetch(e)) return rc;
    if (st.w[TW_RANGE])
        return raft_internal_fail(RAFT_ERANGE, "a transfer's group is outside the engine; nothing was written");
    return RAFT_OK;
}

int resolve_dev(raft_engine* e, const int64_t* group, const raft_transfer_ticket* ticket, raft_transfer_state* out, int n) {
    e->fork_needed = true;
    Status st;
    if (int rc = zeroed_status(e, st)) return rc;
    transfer_resolve_kernel<<<(unsigned)((n + BLOCK - 1) / BLOCK), BLOCK, 0, e->stream>>>(
        e->dp, group, (const int4*)ticket, (int4*)out, n, st.dev);
    HIP_TRY(hipGetLastError());
    if (int rc = st.fetch(e)) return rc;
    if (st.w[TW_RANGE])
        return raft_internal_fail(RAFT_ERANGE, "a transfer ticket's group is outside the engine (its record is INVALID)");
    if (st.w[TW_INVAL])
        return raft_internal_fail(RAFT_EINVAL, "a SENT ticket's from or target is outside the engine (its record is INVALID)");
    return RAFT_OK;
}

int evacuate(raft_engine* e, int64_t g0, int64_t n, bool host, const uint8_t* mask, raft_evacuate_info* info) {
    if (!e) return raft_internal_fail(RAFT_EINVAL, "null engine");
    if (!info) return raft_internal_fail(RAFT_EINVAL, "null info");
    *info = raft_evacuate_info{};
    if (int rc = check_groups(e, g0, n)) return rc;
    if (n == 0) return RAFT_OK;
    if (!mask) return raft_internal_fail(RAFT_EINVAL, "null mask");
    HIP_TRY(hipSetDevice(e->device));
    e->fork_needed = true;                           // later step launches wait for the timers set here
    raft_internal_ensure_cache(e);
    // staging: the counts, then the device copy of a host mask
    if (int rc = raft_internal_grow_dev(e, &e->aux, &e->aux_bytes, Counts::BYTES + (host ? (size_t)n : 0))) return rc;
    Counts c;
    if (int rc = c.zero(e, e->aux)) return rc;
    if (host) {
        HIP_TRY(hipMemcpyAsync(e->aux + Counts::BYTES, mask, (size_t)n, hipMemcpyHostToDevice, e->stream));
        mask = (const uint8_t*)(e->aux + Counts::BYTES);
    }
    evacuate_kernel<<<(unsigned)((n + BLOCK - 1) / BLOCK), BLOCK, 0, e->stream>>>(e->dp, g0, n, mask, c.dev);
    HIP_TRY(hipGetLastError());
    if (int rc = c.fetch(e)) return rc;
    info->led = (int64_t)c.w[EV_LED];
    info->sent = (int64_t)c.w[EV_SENT];
    info->no_target = (int64_t)c.w[EV_NO_TARGET];
    info->behind = (int64_t)c.w[EV_BEHIND];
    info->busy = (int64_t)c.w[EV_BUSY];
    return RAFT_OK;
}

}  // namespace

extern "C" {

int raft_transfer_batch_dev(raft_engine* e, const int64_t* group, const int32_t* target, raft_transfer_ticket* ticket,
                            int64_t n) {
    if (int rc = check_args(e, n, !group || !target || !ticket)) return rc;
    if (n == 0) return RAFT_OK;
    if (!aligned16(ticket)) return raft_internal_fail(RAFT_EINVAL, "the ticket buffer must be 16-byte aligned");
    HIP_TRY(hipSetDevice(e->device));
    return transfer_dev(e, group, target, ticket, (int)n);
}

int raft_transfer_batch(raft_engine* e, const int64_t* group, const int32_t* target, raft_transfer_ticket* ticket,
                        int64_t n) {
    if (int rc = check_args(e, n, !group || !target || !ticket)) return rc;
    if (n == 0) return RAFT_OK;
    HIP_TRY(hipSetDevice(e->device));
    const void* src[2] = {group, target};
    const size_t bytes[2] = {(size_t)n * 8, (size_t)n * 4};
    Staged s;
    if (int rc = stage_in(e, src, bytes, 2, (size_t)n * sizeof(raft_transfer_ticket), s)) return rc;
    if (int rc = transfer_dev(e, (const int64_t*)(e->cio + s.off[0]), (const int32_t*)(e->cio + s.off[1]),
                              (raft_transfer_ticket*)(e->cio + s.out_off), (int)n))
        return rc;                                                      // RAFT_ERANGE: no ticket was written
    return stage_out(e, s, ticket);
}

int raft_engine_resolve_transfers_dev(raft_engine* e, const int64_t* group, const raft_transfer_ticket* ticket,
                                      raft_transfer_state* out, int64_t n) {
    if (int rc = check_args(e, n, !group || !ticket || !out)) return rc;
    if (n == 0) return RAFT_OK;
    if (!aligned16(ticket) || !aligned16(out))
        return raft_internal_fail(RAFT_EINVAL, "the ticket and record buffers must be 16-byte aligned");
    HIP_TRY(hipSetDevice(e->device));
    return resolve_dev(e, group, ticket, out, (int)n);
}

int raft_engine_resolve_transfers(raft_engine* e, const int64_t* group, const raft_transfer_ticket* ticket,
                                  raft_transfer_state* out, int64_t n) {
    if (int rc = check_args(e, n, !group || !ticket || !out)) return rc;
    if (n == 0) return RAFT_OK;
    HIP_TRY(hipSetDevice(e->device));
    const void* src[2] = {group, ticket};
    const size_t bytes[2] = {(size_t)n * 8, (size_t)n * sizeof(raft_transfer_ticket)};
    Staged s;
    if (int rc = stage_in(e, src, bytes, 2, (size_t)n * sizeof(raft_transfer_state), s)) return rc;
    const int rc = resolve_dev(e, (const int64_t*)(e->cio + s.off[0]), (const raft_transfer_ticket*)(e->cio + s.off[1]),
                               (raft_transfer_state*)(e->cio + s.out_off), (int)n);
    if (rc == RAFT_EDEVICE || rc == RAFT_ENOMEM) return rc;
    if (int rc2 = stage_out(e, s, out)) return rc2;                     // every record is filled, whatever rc says
    return rc;
}

int raft_engine_evacuate(raft_engine* e, int64_t g0, int64_t n, const uint8_t* mask_host, raft_evacuate_info* info) {
    return evacuate(e, g0, n, true, mask_host, info);
}

int raft_engine_evacuate_dev(raft_engine* e, int64_t g0, int64_t n, const uint8_t* mask_dev, raft_evacuate_info* info) {
    return evacuate(e, g0, n, false, mask_dev, info);
}

}  // extern "C"
