// raft_client.hip — the client path (include/raft_engine.h
// raft_engine_read_leaders, raft_propose_batch*, raft_engine_resolve_tickets*):
// what an outside client of the reference does through one node's
// /cmd/{command} route (RaftServer.kt:87-88, appendCommand :100-107), for many
// groups at once, and the answer the reference never gives: where the entry
// went and whether it committed.
//
// Kernels of its own, beside the handler batches (raft_batch.hip) and the
// drain (raft_apply.hip); the step kernel, the canonical state and the digest
// do not know about any of it.
//   leaders   one thread per group: the R role words (quad 0 of each replica),
//             then the chosen leader's commitIndex
//   propose   keys (the group of each message), a stable radix sort of (group,
//             message index) -- so a group's messages stay in batch order --
//             then one thread per run head: it routes (the run's one read of the
//             R role words), loads the leader's quads 0-2 once, applies the
//             run with raft_step.h's append_command, writes each message's
//             ticket and stores back the quads that changed (quads 1 and 2)
//   resolve   read-only; eight lanes per ticket, lane r for replica r: its
//             lastIndex / physLen (quad 1), commitIndex (quad 2) and the one
//             8-byte log slot the ticket names; the counts are reduced over the
//             eight lanes by shuffles and lane 0 stores the 16-byte record
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>

#include <string>

#include "raft_engine_impl.h"
#include "raft_ticket.h"

using namespace raft;

namespace {

static_assert(sizeof(raft_leader_info) == 16 && sizeof(raft_ticket) == 16 && sizeof(raft_ticket_state) == 16,
              "record layouts of the C-ABI");

// status words of a call (DevWords, raft_engine_impl.h: one stripe), at the head of cli
enum { CW_RANGE = 0, CW_MISS = 1, CW_INVAL = 2, CW_UNKNOWN = 3, CW_WORDS = 4 };
constexpr size_t CW_BYTES = 256;
using Status = DevWords<unsigned int, 1, CW_WORDS, CW_WORDS, false>;

// (the group's leader, find_leader: raft_engine_impl.h)
__global__ __launch_bounds__(BLOCK) void leaders_kernel(DevParams p, int64_t g0, int64_t n, int4* __restrict__ out) {
    const int64_t j = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n) return;
    const Lead l = find_leader(p, g0 + j);
    const int32_t commit = l.r >= 0 ? quad(p, 2, (g0 + j) * p.R + l.r)->x : 0;
    out[j] = make_int4(l.r, l.term, l.n, commit);                      // raft_leader_info
}

// keys[m] = group[m] (G < 2^31: always a 32-bit key); a group outside the
// engine sets the range word and nothing is applied
__global__ __launch_bounds__(BLOCK) void propose_keys_kernel(const int64_t* __restrict__ group, int n, int64_t G,
                                                             uint32_t* __restrict__ keys, uint32_t* __restrict__ ord,
                                                             unsigned int* flags) {
    const int m = blockIdx.x * BLOCK + threadIdx.x;
    if (m >= n) return;
    const int64_t g = group[m];
    const bool ok = g >= 0 && g < G;
    keys[m] = ok ? (uint32_t)g : 0u;
    ord[m] = (uint32_t)m;
    if (!ok) atomicOr(&flags[CW_RANGE], 1u);
}

// One thread per sorted position; the first position of each group's run
// routes and applies the run (batch_kernel's shape, raft_batch.hip).
// LOG_FULL and GHOSTED are read off lastIndex and physLen around the add:
// a refused add leaves lastIndex alone, and the reference's add lands on the
// physical end, which is slot lastIndex only when the two were equal (Q1).
template <bool TB>
__global__ __launch_bounds__(BLOCK) void propose_kernel(DevParams p, int n, const uint32_t* __restrict__ keys,
                                                        const uint32_t* __restrict__ order,
                                                        const uint32_t* __restrict__ cmd, int4* __restrict__ ticket,
                                                        unsigned int* flags) {
    const int m0 = blockIdx.x * BLOCK + threadIdx.x;
    if (m0 >= n || *(volatile unsigned int*)&flags[CW_RANGE]) return;
    const uint32_t key = keys[m0];
    if (m0 > 0 && keys[m0 - 1] == key) return;                          // not the first of its run
    auto more = [&](int m) { return m < n && keys[m] == key; };
    const Lead l = find_leader(p, (int64_t)key);
    if (l.r < 0) {                                                      // nothing is appended
        for (int m = m0; more(m); ++m) ticket[order[m]] = make_int4(-1, -1, 0, RAFT_PROPOSE_NO_LEADER);
        return;
    }
    const int64_t idx = (int64_t)key * p.R + l.r;
    // the run's first command is fetched with the replica's fields; each later
    // one while the previous message is applied (apply_run's pipeline)
    uint32_t om = order[m0];
    uint32_t c = cmd[om];
    RepState x;
    RepQuads o;
    load_rep(x, o, p, idx);
    const LogView lv = log_of(p, idx);
    BatchCounters cnt;
    for (int m = m0;;) {
        const uint32_t cm = c, oc = om;
        const bool next = more(m + 1);
        if (next) {
            om = order[m + 1];
            c = cmd[om];
        }
        const int32_t last0 = x.last, phys0 = x.phys;
        append_command<TB, true>(x.ref(), __ballot(1), lv, cm, cnt);
        const int32_t st = x.last == last0              ? RAFT_PROPOSE_LOG_FULL
                           : (!TB && phys0 != last0)   ? RAFT_PROPOSE_GHOSTED
                                                       : RAFT_PROPOSE_ACCEPTED;
        ticket[oc] = make_int4(l.r, last0, x.term, st);                 // raft_ticket
        ++m;
        if (!next) break;
    }
    store_rep(x, o, p, idx);
    if (cnt.miss) atomicAdd(&flags[CW_MISS], cnt.miss);
}

// Eight lanes per ticket (RAFT_MAX_R), lanes >= R idle.  Every lane of a wave
// stays in the kernel to the end (the shuffles read all eight lanes of a
// ticket); lanes past the last ticket read the last one and store nothing.
__global__ __launch_bounds__(BLOCK) void resolve_kernel(DevParams p, const int64_t* __restrict__ group,
                                                        const int4* __restrict__ ticket,
                                                        const uint32_t* __restrict__ cmd, int4* __restrict__ out,
                                                        int64_t n, unsigned int* flags) {
    const int64_t tid = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const int r = (int)(tid & 7);
    const bool live = (tid >> 3) < n;
    const int64_t m = live ? tid >> 3 : n - 1;
    const int64_t g = group[m];
    const int4 tk = ticket[m];                                          // (replica, index, term, status)
    const uint32_t c = cmd[m];
    const bool stored = tk.w != RAFT_PROPOSE_NO_LEADER && tk.w != RAFT_PROPOSE_LOG_FULL;
    // (the per-ticket routine, shared with the outbox's verdict pass: raft_ticket.h)
    const uint32_t v = ticket_sum(ticket_lane(p, g, tk, c, r, stored));
    if (!live || r != 0) return;
    const TicketVerdict o = ticket_verdict(p, g, tk, stored, v);
    if (!o.g_ok) atomicOr(&flags[CW_RANGE], 1u);
    else if (stored && !o.t_ok) atomicOr(&flags[CW_INVAL], 1u);
    else if (o.status == RAFT_TICKET_UNKNOWN) atomicOr(&flags[CW_UNKNOWN], 1u);
    out[m] = make_int4(o.status, o.holders, o.committed_on, o.unknown); // raft_ticket_state
}

// (the sort's configuration, SortConfig: raft_engine_impl.h)
int propose_enqueue(raft_engine* e, const int64_t* group, const uint32_t* cmd, raft_ticket* ticket, int n) {
    e->fork_needed = true;
    raft_internal_ensure_cache(e);                  // append_command reads and writes the HBM tail cache
    int bits = 1;
    while (bits < 32 && ((uint64_t)e->p.G - 1) >> bits) ++bits;
    size_t sort_tmp = 0;
    HIP_TRY(rocprim::radix_sort_pairs<SortConfig>(nullptr, sort_tmp, (const uint32_t*)nullptr, (uint32_t*)nullptr,
                                                  (const uint32_t*)nullptr, (uint32_t*)nullptr, n, 0u, (unsigned)bits,
                                                  e->stream));
    const size_t b_n = al256((size_t)n * 4);
    if (int rc = raft_internal_grow_dev(e, &e->cli, &e->cli_bytes, CW_BYTES + 4 * b_n + al256(sort_tmp))) return rc;
    Status st;
    uint32_t* k_in = (uint32_t*)(e->cli + CW_BYTES);
    uint32_t* k_out = (uint32_t*)(e->cli + CW_BYTES + b_n);
    uint32_t* o_in = (uint32_t*)(e->cli + CW_BYTES + 2 * b_n);
    uint32_t* o_out = (uint32_t*)(e->cli + CW_BYTES + 3 * b_n);
    void* tmp = e->cli + CW_BYTES + 4 * b_n;
    if (int rc = st.zero(e, e->cli)) return rc;
    const unsigned grid = (unsigned)((n + BLOCK - 1) / BLOCK);
    propose_keys_kernel<<<grid, BLOCK, 0, e->stream>>>(group, n, e->p.G, k_in, o_in, st.dev);
    HIP_TRY(rocprim::radix_sort_pairs<SortConfig>(tmp, sort_tmp, k_in, k_out, o_in, o_out, n, 0u, (unsigned)bits,
                                                  e->stream));
    if (e->p.mode == RAFT_MODE_TEXTBOOK)
        propose_kernel<true><<<grid, BLOCK, 0, e->stream>>>(e->dp, n, k_out, o_out, cmd, (int4*)ticket, st.dev);
    else
        propose_kernel<false><<<grid, BLOCK, 0, e->stream>>>(e->dp, n, k_out, o_out, cmd, (int4*)ticket, st.dev);
    HIP_TRY(hipGetLastError());
    return RAFT_OK;
}

// the status words of the propose enqueued last, at the head of cli
int propose_finish(raft_engine* e) {
    Status st;
    st.dev = (unsigned int*)e->cli;
    if (int rc = st.fetch(e)) return rc;
    if (st.w[CW_RANGE])
        return raft_internal_fail(RAFT_ERANGE, "a proposal's group is outside the engine; nothing was applied");
    if (st.w[CW_MISS])
        return raft_internal_fail(RAFT_EWINDOW, std::to_string(st.w[CW_MISS]) +
                                                    " log accesses below the retained log_window: the batch's "
                                                    "results are not the reference's");
    return RAFT_OK;
}

int propose_dev(raft_engine* e, const int64_t* group, const uint32_t* cmd, raft_ticket* ticket, int n) {
    if (int rc = propose_enqueue(e, group, cmd, ticket, n)) return rc;
    return propose_finish(e);
}

int resolve_dev(raft_engine* e, const int64_t* group, const raft_ticket* ticket, const uint32_t* cmd,
                raft_ticket_state* out, int64_t n) {
    e->fork_needed = true;                          // later step launches wait for these reads of the state and logs
    if (int rc = raft_internal_grow_dev(e, &e->cli, &e->cli_bytes, CW_BYTES)) return rc;
    Status st;
    if (int rc = st.zero(e, e->cli)) return rc;
    const unsigned grid = (unsigned)((n * RAFT_MAX_R + BLOCK - 1) / BLOCK);
    resolve_kernel<<<grid, BLOCK, 0, e->stream>>>(e->dp, group, (const int4*)ticket, cmd, (int4*)out, n, st.dev);
    HIP_TRY(hipGetLastError());
    if (int rc = st.fetch(e)) return rc;
    if (st.w[CW_RANGE])
        return raft_internal_fail(RAFT_ERANGE, "a ticket's group is outside the engine (its record is INVALID)");
    if (st.w[CW_INVAL])
        return raft_internal_fail(RAFT_EINVAL, "a ticket's replica or index is outside the engine (its record is INVALID)");
    if (st.w[CW_UNKNOWN])
        return raft_internal_fail(RAFT_EWINDOW, "a ticket's slot is below a replica's log_window (its record is UNKNOWN)");
    return RAFT_OK;
}

}  // namespace

// (raft_ticket.h: the outbox's re-propose)
int raft_internal_propose_enqueue(raft_engine* e, const int64_t* group, const uint32_t* cmd, raft_ticket* ticket, int n) {
    return propose_enqueue(e, group, cmd, ticket, n);
}
int raft_internal_propose_finish(raft_engine* e) { return propose_finish(e); }

extern "C" {

int raft_engine_read_leaders(raft_engine* e, int64_t g0, int64_t n, raft_leader_info* out_host) {
    if (int rc = check_groups(e, g0, n)) return rc;
    if (n == 0) return RAFT_OK;
    if (!out_host) return raft_internal_fail(RAFT_EINVAL, "null buffer");
    HIP_TRY(hipSetDevice(e->device));
    e->fork_needed = true;
    if (int rc = raft_internal_grow_dev(e, &e->cio, &e->cio_bytes, (size_t)n * sizeof(raft_leader_info))) return rc;
    leaders_kernel<<<(unsigned)((n + BLOCK - 1) / BLOCK), BLOCK, 0, e->stream>>>(e->dp, g0, n, (int4*)e->cio);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out_host, e->cio, (size_t)n * sizeof(raft_leader_info), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return RAFT_OK;
}

int raft_propose_batch_dev(raft_engine* e, const int64_t* group, const uint32_t* cmd, raft_ticket* ticket, int64_t n) {
    if (int rc = check_args(e, n, !group || !cmd || !ticket)) return rc;
    if (n == 0) return RAFT_OK;
    if (!aligned16(ticket)) return raft_internal_fail(RAFT_EINVAL, "the ticket buffer must be 16-byte aligned");
    HIP_TRY(hipSetDevice(e->device));
    return propose_dev(e, group, cmd, ticket, (int)n);
}

int raft_propose_batch(raft_engine* e, const int64_t* group, const uint32_t* cmd, raft_ticket* ticket, int64_t n) {
    if (int rc = check_args(e, n, !group || !cmd || !ticket)) return rc;
    if (n == 0) return RAFT_OK;
    HIP_TRY(hipSetDevice(e->device));
    const void* src[2] = {group, cmd};
    const size_t bytes[2] = {(size_t)n * 8, (size_t)n * 4};
    Staged s;
    if (int rc = stage_in(e, src, bytes, 2, (size_t)n * sizeof(raft_ticket), s)) return rc;
    const int rc = propose_dev(e, (const int64_t*)(e->cio + s.off[0]), (const uint32_t*)(e->cio + s.off[1]),
                               (raft_ticket*)(e->cio + s.out_off), (int)n);
    if (rc != RAFT_OK && rc != RAFT_EWINDOW) return rc;
    if (int rc2 = stage_out(e, s, ticket)) return rc2;
    return rc;
}

int raft_engine_resolve_tickets_dev(raft_engine* e, const int64_t* group, const raft_ticket* ticket,
                                    const uint32_t* cmd, raft_ticket_state* out, int64_t n) {
    if (int rc = check_args(e, n, !group || !ticket || !cmd || !out)) return rc;
    if (n == 0) return RAFT_OK;
    if (!aligned16(ticket) || !aligned16(out))
        return raft_internal_fail(RAFT_EINVAL, "the ticket and record buffers must be 16-byte aligned");
    HIP_TRY(hipSetDevice(e->device));
    return resolve_dev(e, group, ticket, cmd, out, n);
}

int raft_engine_resolve_tickets(raft_engine* e, const int64_t* group, const raft_ticket* ticket, const uint32_t* cmd,
                                raft_ticket_state* out, int64_t n) {
    if (int rc = check_args(e, n, !group || !ticket || !cmd || !out)) return rc;
    if (n == 0) return RAFT_OK;
    HIP_TRY(hipSetDevice(e->device));
    const void* src[3] = {group, ticket, cmd};
    const size_t bytes[3] = {(size_t)n * 8, (size_t)n * sizeof(raft_ticket), (size_t)n * 4};
    Staged s;
    if (int rc = stage_in(e, src, bytes, 3, (size_t)n * sizeof(raft_ticket_state), s)) return rc;
    const int rc = resolve_dev(e, (const int64_t*)(e->cio + s.off[0]), (const raft_ticket*)(e->cio + s.off[1]),
                               (const uint32_t*)(e->cio + s.off[2]), (raft_ticket_state*)(e->cio + s.out_off), n);
    if (rc == RAFT_EDEVICE || rc == RAFT_ENOMEM) return rc;
    if (int rc2 = stage_out(e, s, out)) return rc2;                     // every record is filled, whatever rc says
    return rc;
}

}  // extern "C"
