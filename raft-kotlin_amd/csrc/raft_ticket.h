// raft_ticket.h — what raft_client.hip (raft_engine_resolve_tickets*) and
// raft_outbox.hip (the proposal outbox's verdict pass) share: the per-ticket
// device routine of a resolve, eight lanes per ticket, and the propose's device
// path as two host calls.  Kept out of raft_engine_impl.h: the step kernel's
// translation unit includes that one.
#pragma once
#include "raft_engine_impl.h"

namespace {

// a resolve's record for one ticket, from the lanes' sum
struct TicketVerdict {
    int32_t status, holders, committed_on, unknown;   // raft_ticket_state
    bool g_ok, t_ok;                                   // (INVALID: which of the two checks failed)
};

// Lane r (0..7) of a ticket's eight: replica r's lastIndex / physLen (quad 1),
// commitIndex (quad 2) and the one 8-byte log slot the ticket names.  `stored`:
// the ticket's status says an entry was written.  Returns
// holder | committed << 8 | unknown << 16 | own << 24 of this replica; lanes
// r >= R, a group outside the engine and a ticket outside it read nothing.
__device__ __forceinline__ uint32_t ticket_lane(const DevParams& p, int64_t g, int4 tk, uint32_t c, int r, bool stored) {
    static_assert(RAFT_MAX_R == 8, "eight lanes per ticket");
    const bool g_ok = g >= 0 && g < p.G;
    // the index is checked against log_cap before any slot is read, and masked in a ring (LogView::at)
    const bool t_ok = tk.x >= -1 && tk.x < p.R && tk.y >= 0 && tk.y < p.cap;
    uint32_t v = 0;
    if (g_ok && stored && t_ok && r < p.R) {
        const int64_t idx = g * p.R + r;
        const int4 q1 = *quad(p, 1, idx);                               // lastIndex, physLen
        const int32_t commit = quad(p, 2, idx)->x;
        const int32_t last = q1.x, phys = q1.y, i = tk.y;
        if (p.W != FLAT_W && i < phys - p.W) {
            v = 1u << 16;                                               // below the window: not read
        } else if (i < last) {
            const uint2 en = *log_of(p, idx).at<true>(i);
            if ((int32_t)en.x == tk.z && en.y == c) {
                const int32_t hi = committed_hi(p, commit, last);
                v = 1u | (i < hi ? 1u << 8 : 0u) | (r == tk.x ? 1u << 24 : 0u);
            }
        }
    }
    return v;
}

// the sum over a ticket's eight lanes (every lane of the wave takes part)
__device__ __forceinline__ uint32_t ticket_sum(uint32_t v) {
#pragma unroll
    for (int d = 1; d < 8; d <<= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// the record of include/raft_engine.h raft_engine_resolve_tickets, rule by rule
__device__ __forceinline__ TicketVerdict ticket_verdict(const DevParams& p, int64_t g, int4 tk, bool stored, uint32_t v) {
    TicketVerdict o;
    o.g_ok = g >= 0 && g < p.G;
    o.t_ok = tk.x >= -1 && tk.x < p.R && tk.y >= 0 && tk.y < p.cap;
    o.holders = (int32_t)(v & 255u);
    o.committed_on = (int32_t)((v >> 8) & 255u);
    o.unknown = (int32_t)((v >> 16) & 255u);
    if (!o.g_ok) o.status = RAFT_TICKET_INVALID;
    else if (!stored) o.status = RAFT_TICKET_NONE;
    else if (!o.t_ok) o.status = RAFT_TICKET_INVALID;
    else if (o.committed_on >= 1) o.status = RAFT_TICKET_COMMITTED;
    else if (o.unknown >= 1) o.status = RAFT_TICKET_UNKNOWN;
    else o.status = (v >> 24) ? RAFT_TICKET_PENDING : RAFT_TICKET_LOST;
    return o;
}

}  // namespace

// raft_client.hip: raft_propose_batch_dev's device path in two halves.  enqueue
// puts the keys, the sort and the propose kernel of n > 0 messages (DEVICE
// arrays) on the engine stream; finish waits for the stream, reads the call's
// status words back and returns raft_propose_batch's code.  A caller may
// enqueue kernels of its own that read the tickets in between.
int raft_internal_propose_enqueue(raft_engine* e, const int64_t* group, const uint32_t* cmd, raft_ticket* ticket, int n);
int raft_internal_propose_finish(raft_engine* e);
