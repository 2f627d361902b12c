// raft_read.hip — linearizable reads (include/raft_engine.h
// raft_read_begin_batch*, raft_read_serve_batch*): Raft's ReadIndex protocol
// (Ongaro's thesis §6.4) shaped like the client path's propose / resolve pair.
// begin names the group's newest leader, its term and its committed prefix;
// serve confirms that leader against the group's term words -- the heartbeat
// round of the protocol, read from HBM -- and answers from its machine once the
// machine has applied that prefix.
//
// Kernels of its own, beside the client path (raft_client.hip) and the state
// machine (raft_sm.hip); both calls only read the canonical state, the logs and
// the machine, and write the caller's records.
//   range   one thread per message: its group against the engine (begin only:
//           a group outside the engine fails the batch before a ticket is written)
//   begin   one thread per message: the R role / term words (quad 0 of each
//           replica), quads 1 and 2 of the newest leader, the 8-byte log slot
//           below its committed prefix; one 16-byte store
//   serve   one thread per message: the R term words, the ticket's replica's
//           head and the register the key names, all in flight at once; one
//           16-byte store
// The status words (range, malformed, window) are OR-ed once per wave, after a
// ballot, into the wave's stripe of 64.
#include <hip/hip_runtime.h>

#include <string>

#include "raft_engine_impl.h"

using namespace raft;

namespace {

static_assert(sizeof(raft_read_ticket) == 16 && sizeof(raft_read_result) == 16, "record layouts of the C-ABI");

// The status words of a call, as RW_STRIPES stripes of one 64-byte line each
// (words 0..2 of a line): a wave ORs into stripe (its index mod RW_STRIPES) and
// the host ORs the stripes (DevWords, raft_engine_impl.h, says why), at the
// head of cli.
enum { RW_RANGE = 0, RW_INVAL = 1, RW_WINDOW = 2, RW_WORDS = 3, RW_LINE = 16, RW_STRIPES = 64 };
using Status = DevWords<unsigned int, RW_STRIPES, RW_LINE, RW_WORDS, false>;

// OR 1 into status word `w` of the wave's stripe, once per wave: every lane of
// the wave calls this.  The range word stays in stripe 0, where the begin pass
// reads it: a group outside the engine fails the call, whatever it costs.
__device__ __forceinline__ void wave_flag(unsigned int* flags, int w, bool mine) {
    const unsigned long long any = __ballot(mine);
    const unsigned stripe = w == RW_RANGE ? 0u : (blockIdx.x * WAVES_PER_BLOCK + (threadIdx.x >> 6)) & (RW_STRIPES - 1);
    if ((threadIdx.x & 63) == 0 && any) atomicOr(&flags[stripe * RW_LINE + w], 1u);
}

__global__ __launch_bounds__(BLOCK) void read_range_kernel(const int64_t* __restrict__ group, int n, int64_t G,
                                                           unsigned int* flags) {
    const int m = blockIdx.x * BLOCK + threadIdx.x;
    const bool live = m < n;
    const int64_t g = group[live ? m : n - 1];
    wave_flag(flags, RW_RANGE, live && (g < 0 || g >= G));
}

// (the group's newest leader, find_newest_leader: raft_engine_impl.h)
__global__ __launch_bounds__(BLOCK) void read_begin_kernel(DevParams p, const int64_t* __restrict__ group,
                                                           int4* __restrict__ ticket, int n, unsigned int* flags) {
    if (*(volatile unsigned int*)&flags[RW_RANGE]) return;             // a group outside the engine: no ticket is written
    const int m = blockIdx.x * BLOCK + threadIdx.x;
    const bool live = m < n;
    const int64_t g = group[live ? m : n - 1];
    bool below = false;
    if (live && g >= 0 && g < p.G) {                                    // (the range word was clear: every group is inside)
        const Lead l = find_newest_leader(p, g);
        int4 tk = make_int4(-1, 0, -1, RAFT_READ_NO_LEADER);            // raft_read_ticket
        if (l.r >= 0) {
            const int64_t idx = g * p.R + l.r;
            const int4 q1 = *quad(p, 1, idx);                           // lastIndex, physLen
            const int32_t commit = quad(p, 2, idx)->x;
            const int32_t hi = committed_hi(p, commit, q1.x);
            int32_t st;
            if (hi == 0) {
                st = RAFT_READ_TERM_UNCOMMITTED;
            } else if (p.W != FLAT_W && hi - 1 < q1.y - p.W) {
                st = RAFT_READ_UNKNOWN;                                 // below the window: not read
                below = true;
            } else {
                // 0 <= hi - 1 < log_cap, and masked in a ring (LogView::at): inside the row
                const uint2 en = *log_of(p, idx).at<true>(hi - 1);
                st = (int32_t)en.x == l.term ? RAFT_READ_ISSUED : RAFT_READ_TERM_UNCOMMITTED;
            }
            tk = make_int4(l.r, l.term, hi, st);
        }
        ticket[m] = tk;
    }
    wave_flag(flags, RW_WINDOW, below);
}

// The ticket's replica and read_index are checked before either is used as an
// index, and the loads of a refused message are not issued at all.
__global__ __launch_bounds__(BLOCK) void read_serve_kernel(DevParams p, int S, const int4* __restrict__ heads,
                                                           const uint32_t* __restrict__ regs,
                                                           const int64_t* __restrict__ group,
                                                           const int4* __restrict__ ticket,
                                                           const uint32_t* __restrict__ key, int4* __restrict__ out, int n,
                                                           unsigned int* flags) {
    const int m = blockIdx.x * BLOCK + threadIdx.x;
    const bool live = m < n;
    const int mm = live ? m : n - 1;
    const int64_t g = group[mm];
    const int4 tk = ticket[mm];                                         // (replica, term, read_index, status)
    const uint32_t k = key[mm];
    const bool g_ok = g >= 0 && g < p.G;
    const bool t_ok = tk.x >= 0 && tk.x < p.R && tk.z >= 0 && tk.z <= p.cap;
    int4 rec = make_int4(0, RAFT_READ_INVALID, 0, 0);                   // raft_read_result: value, status, applied, agree
    if (live && g_ok && t_ok) {
        if (tk.w != RAFT_READ_ISSUED) {
            rec.y = RAFT_READ_NONE;
        } else {
            const int R = p.R;
            int4 q[RAFT_MAX_R];
            load_roles(p, g, q);
            const int64_t idx = g * R + tk.x;
            const int4 hd = heads[idx];                                 // applied, lost, hash
            const uint32_t v = regs[idx * S + (k & (uint32_t)(S - 1))];
            int32_t agree = 0;
            bool leads = false;
#pragma unroll
            for (int r = 0; r < RAFT_MAX_R; ++r) {
                const bool same = r < R && q[r].x == tk.y;
                agree += same ? 1 : 0;
                leads |= same && r == tk.x && q[r].z == RAFT_LEADER;
            }
            rec.w = agree;
            if (!leads) {
                rec.y = RAFT_READ_DEPOSED;
            } else if (agree < R / 2 + 1) {
                rec.y = RAFT_READ_NO_QUORUM;
            } else {
                rec.z = hd.x;
                if (hd.x < tk.z) {
                    rec.y = RAFT_READ_BEHIND;
                } else if (hd.y != 0) {
                    rec.y = RAFT_READ_GAPPED;
                } else {
                    rec.y = RAFT_READ_SERVED;
                    rec.x = (int32_t)v;
                }
            }
        }
    }
    if (live) out[m] = rec;
    wave_flag(flags, RW_RANGE, live && !g_ok);
    wave_flag(flags, RW_INVAL, live && g_ok && !t_ok);
}

int zeroed_status(raft_engine* e, Status& st) {
    if (int rc = raft_internal_grow_dev(e, &e->cli, &e->cli_bytes, Status::BYTES)) return rc;
    return st.zero(e, e->cli);
}

int begin_dev(raft_engine* e, const int64_t* group, raft_read_ticket* ticket, int n) {
    e->fork_needed = true;                          // later step launches wait for these reads of the state and logs
    Status st;
    if (int rc = zeroed_status(e, st)) return rc;
    const unsigned grid = (unsigned)((n + BLOCK - 1) / BLOCK);
    read_range_kernel<<<grid, BLOCK, 0, e->stream>>>(group, n, e->p.G, st.dev);
    read_begin_kernel<<<grid, BLOCK, 0, e->stream>>>(e->dp, group, (int4*)ticket, n, st.dev);
    HIP_TRY(hipGetLastError());
    if (int rc = st.fetch(e)) return rc;
    if (st.w[RW_RANGE])
        return raft_internal_fail(RAFT_ERANGE, "a read's group is outside the engine; no ticket was written");
    if (st.w[RW_WINDOW])
        return raft_internal_fail(RAFT_EWINDOW, "a leader's last committed slot is below its log_window (its ticket is UNKNOWN)");
    return RAFT_OK;
}

int serve_dev(raft_engine* e, const int64_t* group, const raft_read_ticket* ticket, const uint32_t* key,
              raft_read_result* out, int n) {
    e->fork_needed = true;
    Status st;
    if (int rc = zeroed_status(e, st)) return rc;
    read_serve_kernel<<<(unsigned)((n + BLOCK - 1) / BLOCK), BLOCK, 0, e->stream>>>(
        e->dp, e->sm_slots, sm_heads_of(e), sm_regs_of(e), group, (const int4*)ticket, key, (int4*)out, n, st.dev);
    HIP_TRY(hipGetLastError());
    if (int rc = st.fetch(e)) return rc;
    if (st.w[RW_RANGE])
        return raft_internal_fail(RAFT_ERANGE, "a read's group is outside the engine (its record is INVALID)");
    if (st.w[RW_INVAL])
        return raft_internal_fail(RAFT_EINVAL, "a ticket's replica or read_index is outside the engine (its record is INVALID)");
    return RAFT_OK;
}

}  // namespace

extern "C" {

int raft_read_begin_batch_dev(raft_engine* e, const int64_t* group, raft_read_ticket* ticket, int64_t n) {
    if (int rc = check_args(e, n, !group || !ticket)) return rc;
    if (n == 0) return RAFT_OK;
    if (!aligned16(ticket)) return raft_internal_fail(RAFT_EINVAL, "the ticket buffer must be 16-byte aligned");
    HIP_TRY(hipSetDevice(e->device));
    return begin_dev(e, group, ticket, (int)n);
}

int raft_read_begin_batch(raft_engine* e, const int64_t* group, raft_read_ticket* ticket, int64_t n) {
    if (int rc = check_args(e, n, !group || !ticket)) return rc;
    if (n == 0) return RAFT_OK;
    HIP_TRY(hipSetDevice(e->device));
    const void* src[1] = {group};
    const size_t bytes[1] = {(size_t)n * 8};
    Staged s;
    if (int rc = stage_in(e, src, bytes, 1, (size_t)n * sizeof(raft_read_ticket), s)) return rc;
    const int rc = begin_dev(e, (const int64_t*)(e->cio + s.off[0]), (raft_read_ticket*)(e->cio + s.out_off), (int)n);
    if (rc != RAFT_OK && rc != RAFT_EWINDOW) return rc;                 // RAFT_ERANGE: no ticket was written
    if (int rc2 = stage_out(e, s, ticket)) return rc2;
    return rc;
}

int raft_read_serve_batch_dev(raft_engine* e, const int64_t* group, const raft_read_ticket* ticket, const uint32_t* key,
                              raft_read_result* out, int64_t n) {
    if (int rc = check_args(e, n, !group || !ticket || !key || !out)) return rc;
    if (int rc = check_sm(e)) return rc;
    if (n == 0) return RAFT_OK;
    if (!aligned16(ticket) || !aligned16(out))
        return raft_internal_fail(RAFT_EINVAL, "the ticket and record buffers must be 16-byte aligned");
    HIP_TRY(hipSetDevice(e->device));
    return serve_dev(e, group, ticket, key, out, (int)n);
}

int raft_read_serve_batch(raft_engine* e, const int64_t* group, const raft_read_ticket* ticket, const uint32_t* key,
                          raft_read_result* out, int64_t n) {
    if (int rc = check_args(e, n, !group || !ticket || !key || !out)) return rc;
    if (int rc = check_sm(e)) return rc;
    if (n == 0) return RAFT_OK;
    HIP_TRY(hipSetDevice(e->device));
    const void* src[3] = {group, ticket, key};
    const size_t bytes[3] = {(size_t)n * 8, (size_t)n * sizeof(raft_read_ticket), (size_t)n * 4};
    Staged s;
    if (int rc = stage_in(e, src, bytes, 3, (size_t)n * sizeof(raft_read_result), s)) return rc;
    const int rc = serve_dev(e, (const int64_t*)(e->cio + s.off[0]), (const raft_read_ticket*)(e->cio + s.off[1]),
                             (const uint32_t*)(e->cio + s.off[2]), (raft_read_result*)(e->cio + s.out_off), (int)n);
    if (rc == RAFT_EDEVICE || rc == RAFT_ENOMEM) return rc;
    if (int rc2 = stage_out(e, s, out)) return rc2;                     // every record is filled, whatever rc says
    return rc;
}

}  // extern "C"
