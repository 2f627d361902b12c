// raft_noop.hip — leader no-op entries (include/raft_engine.h
// raft_engine_append_noops*): Raft's rule that a new leader appends an entry of
// its own term (Ongaro's thesis §3.6.2, §6.4 step 1), as a side path between
// two step launches.  The reference has no such entry; the append itself is
// raft_step.h's append_command, the one raft_propose_batch runs.
//
// One kernel, on the plumbing of raft_engine_impl.h:
//   noop   one thread per group of the range: the R role / term words (quad 0
//          of each replica), then quads 0-2 of the newest leader (quad 0 is the
//          sector just read).  The term of the leader's last entry is the
//          log-tail cache's t1, so no log slot is read.  Where the tail is of
//          an older term (or the log is empty): one 8-byte slot store and the
//          quads that changed (quads 1 and 2).  With tickets, one 16-byte and
//          one 4-byte store per group.  The counts are reduced per wave (ballot
//          and popcount) before one atomic per nonzero word into the wave's
//          stripe.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>

#include "raft_stream.h"

using namespace raft;

namespace {

static_assert(sizeof(raft_noop_info) == 64 && sizeof(raft_ticket) == 16, "record layouts of the C-ABI");

// the counts of a call, striped as a restart's totals, at the head of aux; NW_MISS: reference accesses below a
// window (propose's RAFT_EWINDOW rule), not part of the info
enum { NW_APPENDED = 0, NW_CURRENT = 1, NW_NO_LEADER = 2, NW_LOG_FULL = 3, NW_GHOSTED = 4, NW_MISS = 5, NW_WORDS = 6 };
using Counts = DevWords<unsigned long long, HDR_STRIPES, HDR_LINE, NW_WORDS, true>;

// ticket / ticket_cmd: [n] on the device, or both null.  The ticket and status of an append are what
// propose_kernel (raft_client.hip) writes for one message to that replica.
template <bool TB>
__global__ __launch_bounds__(BLOCK) void noop_kernel(DevParams p, int64_t g0, int64_t n, uint32_t cmd,
                                                     int4* __restrict__ ticket, uint32_t* __restrict__ ticket_cmd,
                                                     unsigned long long* hdr) {
    const int64_t j = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const bool live = j < n;
    const int64_t g = g0 + (live ? j : n - 1);                          // g0 <= g < g0 + n <= G (check_groups)
    const Lead l = find_newest_leader(p, g);
    int4 tk = make_int4(-1, -1, 0, RAFT_PROPOSE_NO_LEADER);             // raft_ticket: replica, index, term, status
    uint32_t tc = 0;
    bool miss = false;
    if (live && l.r >= 0) {
        const int64_t idx = g * p.R + l.r;                              // 0 <= l.r < R: inside the state
        RepState x;
        RepQuads o;
        load_rep(x, o, p, idx);
        if (x.last >= 1 && x.t1 == x.term) {                            // the tail entry is of the leader's own term
            tk = make_int4(l.r, x.last - 1, x.term, RAFT_PROPOSE_CURRENT);
            tc = x.c1;
        } else {
            const LogView lv = log_of(p, idx);
            BatchCounters cnt;
            const int32_t last0 = x.last, phys0 = x.phys;
            append_command<TB, true>(x.ref(), __ballot(1), lv, cmd, cnt);
            const int32_t st = x.last == last0              ? RAFT_PROPOSE_LOG_FULL
                               : (!TB && phys0 != last0)   ? RAFT_PROPOSE_GHOSTED
                                                           : RAFT_PROPOSE_ACCEPTED;
            tk = make_int4(l.r, last0, x.term, st);
            tc = cmd;
            store_rep(x, o, p, idx);
            miss = cnt.miss != 0;
        }
    }
    if (live && ticket) {
        ticket[j] = tk;
        ticket_cmd[j] = tc;
    }
    // the counts: one atomic per nonzero word and wave
    const unsigned long long b_cur = __ballot(live && tk.w == RAFT_PROPOSE_CURRENT),
                             b_nol = __ballot(live && tk.w == RAFT_PROPOSE_NO_LEADER),
                             b_full = __ballot(live && tk.w == RAFT_PROPOSE_LOG_FULL),
                             b_gho = __ballot(live && tk.w == RAFT_PROPOSE_GHOSTED),
                             b_app = __ballot(live && (tk.w == RAFT_PROPOSE_ACCEPTED || tk.w == RAFT_PROPOSE_GHOSTED)),
                             b_miss = __ballot(miss);
    if ((threadIdx.x & 63) == 0) {
        unsigned long long* line = stripe_of(hdr, wave_index());
        tally_ballot(line, NW_APPENDED, b_app);
        tally_ballot(line, NW_CURRENT, b_cur);
        tally_ballot(line, NW_NO_LEADER, b_nol);
        tally_ballot(line, NW_LOG_FULL, b_full);
        tally_ballot(line, NW_GHOSTED, b_gho);
        tally_ballot(line, NW_MISS, b_miss);
    }
}

int append_noops(raft_engine* e, int64_t g0, int64_t n, uint32_t cmd, bool host, raft_ticket* ticket,
                 uint32_t* ticket_cmd, raft_noop_info* info) {
    if (!e) return raft_internal_fail(RAFT_EINVAL, "null engine");
    if (!info) return raft_internal_fail(RAFT_EINVAL, "null info");
    *info = raft_noop_info{};
    if ((ticket == nullptr) != (ticket_cmd == nullptr))
        return raft_internal_fail(RAFT_EINVAL, "ticket and ticket_cmd come together: both or neither");
    if (int rc = check_groups(e, g0, n)) return rc;
    if (n == 0) return RAFT_OK;
    if (!host && ticket && !aligned16(ticket))
        return raft_internal_fail(RAFT_EINVAL, "the ticket buffer must be 16-byte aligned");
    HIP_TRY(hipSetDevice(e->device));
    e->fork_needed = true;                           // later step launches wait for the entries appended here
    raft_internal_ensure_cache(e);                   // t1 is compared and append_command keeps the HBM tail cache
    if (int rc = raft_internal_grow_dev(e, &e->aux, &e->aux_bytes, Counts::BYTES)) return rc;
    Counts c;
    if (int rc = c.zero(e, e->aux)) return rc;
    // a host call's records: tickets [n], then ticket_cmd [n], in cio and in the page-locked staging
    const size_t cmd_off = al256((size_t)n * sizeof(raft_ticket)), out_bytes = cmd_off + (size_t)n * 4;
    int4* tk_dev = (int4*)ticket;
    uint32_t* tc_dev = ticket_cmd;
    if (host && ticket) {
        if (int rc = raft_internal_grow_dev(e, &e->cio, &e->cio_bytes, out_bytes)) return rc;
        if (int rc = raft_internal_grow_host(e, &e->hst, &e->hst_bytes, out_bytes)) return rc;
        tk_dev = (int4*)e->cio;
        tc_dev = (uint32_t*)(e->cio + cmd_off);
    }
    const unsigned grid = (unsigned)((n + BLOCK - 1) / BLOCK);
    if (e->p.mode == RAFT_MODE_TEXTBOOK)
        noop_kernel<true><<<grid, BLOCK, 0, e->stream>>>(e->dp, g0, n, cmd, tk_dev, tc_dev, c.dev);
    else
        noop_kernel<false><<<grid, BLOCK, 0, e->stream>>>(e->dp, g0, n, cmd, tk_dev, tc_dev, c.dev);
    HIP_TRY(hipGetLastError());
    if (host && ticket)
        HIP_TRY(hipMemcpyAsync(e->hst, e->cio, out_bytes, hipMemcpyDeviceToHost, e->stream));
    if (int rc = c.fetch(e)) return rc;              // (waits for the records too)
    if (host && ticket) {
        std::memcpy(ticket, e->hst, (size_t)n * sizeof(raft_ticket));
        std::memcpy(ticket_cmd, e->hst + cmd_off, (size_t)n * 4);
    }
    info->appended = (int64_t)c.w[NW_APPENDED];
    info->current = (int64_t)c.w[NW_CURRENT];
    info->no_leader = (int64_t)c.w[NW_NO_LEADER];
    info->log_full = (int64_t)c.w[NW_LOG_FULL];
    info->ghosted = (int64_t)c.w[NW_GHOSTED];
    if (c.w[NW_MISS])
        return raft_internal_fail(RAFT_EWINDOW, std::to_string(c.w[NW_MISS]) +
                                                    " log accesses below the retained log_window: the call's "
                                                    "results are not the reference's");
    return RAFT_OK;
}

}  // namespace

extern "C" {

int raft_engine_append_noops(raft_engine* e, int64_t g0, int64_t n, uint32_t cmd, raft_ticket* ticket_host,
                             uint32_t* ticket_cmd_host, raft_noop_info* info) {
    return append_noops(e, g0, n, cmd, true, ticket_host, ticket_cmd_host, info);
}

int raft_engine_append_noops_dev(raft_engine* e, int64_t g0, int64_t n, uint32_t cmd, raft_ticket* ticket_dev,
                                 uint32_t* ticket_cmd_dev, raft_noop_info* info) {
    return append_noops(e, g0, n, cmd, false, ticket_dev, ticket_cmd_dev, info);
}

}  // extern "C"
