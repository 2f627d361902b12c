// raft_fault.hip — replica crash and restart on the device (include/raft_engine.h
// raft_engine_restart*): the chosen replicas lose their volatile state in HBM,
// and with RAFT_RESTART_AMNESIA the Raft-paper persistent state too.
//
// One kernel for the three entry points (a host mask, a device mask, a seeded
// rate).  A wave holds GPW = 64 / R whole groups, one lane per replica (lane
// (g % GPW) * R + r, as the step kernel and the handler batches place them), so
// everything a group needs -- which of its replicas restart, the lowest of
// them, whether the primary session's owner is among them -- is a slice of one
// wave ballot, and no group word is touched by an atomic.
//   selection  mask: bit r of the group's byte; rate: the replica's
//              RAFT_RNG_RESTART word against the ppm (philox.h hit32, which is
//              w < ceil(ppm * 2^32 / 10^6)).  A wave that selects nothing returns
//              before it reads any state.
//   replica    quad 0 and quad 1 are read (role and lastIndex are counted, and
//              without AMNESIA term, votedFor, lastIndex, physLen, t1 stay);
//              quad 2 only without AMNESIA (t2, c1 stay).  Each is written
//              whole; of quad 3 only retryMs is stored: its other words are the
//              primary session's column towards this replica, another replica's
//              row.  The election timeout is drawn here (the handler batches'
//              resolve_rep_draw at the engine's step index), so no FL_DRAW is left.
//   sessions   rows next[r][*] / match[r][*] of a restarted r become zero, the
//              way write_state leaves canonical rows: in spill.  Every lane d of
//              a group with a restart zeroes its own [d][r] words; if r owned the
//              primary slot, the group's lead lane sets the owner word to -1 and
//              the F_NX / F_MC words it used are dead.
//   consumers  lastApplied and the machine's head: one store per replica.  The
//              machine's registers: the wave walks the selected replicas' S
//              words 64 at a time, a lane finds the replica of its word by a
//              binary search over the ballot's prefix counts (no lane loops
//              over S words).
//   totals     per wave, one atomic per nonzero word into the wave's stripe of
//              a small header (the scheme of sm_apply_kernel); the host sums it.
#include <hip/hip_runtime.h>

#include <string>

#include "raft_stream.h"

using namespace raft;

namespace {

static_assert(sizeof(raft_restart_info) == 32, "record layout of the C-ABI");

// the totals of a restart (Totals, raft_engine_impl.h): these words of a wave's stripe
constexpr int HDR_RESTARTED = 0, HDR_LEADERS = 1, HDR_DROPPED = 2;
constexpr int32_t MAX_DOWN_STEPS = (1 << 23) - 1;

struct RestartArgs {
    int64_t g0, n;                 // groups [g0, g0 + n)
    const uint8_t* mask;           // [n] device bytes, or nullptr: the seeded rate
    uint32_t ppm, t;               // the rate; the engine's step index (Philox c0)
    int32_t flags, down_steps;
    int32_t* applied;              // lastApplied [G * R]
    int4* heads;                   // the machine's heads [G * R], nullptr if not configured
    uint32_t* regs;                // its registers [G * R][1 << logS]
    int32_t logS;
    unsigned long long* hdr;
};

template <int R>
__global__ __launch_bounds__(BLOCK) void restart_kernel(DevParams p, RestartArgs a) {
    constexpr int GPW = 64 / R;
    constexpr uint32_t GROUP_BITS = (1u << R) - 1u;
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * WAVES_PER_BLOCK + (threadIdx.x >> 6);
    const int gl = lane / R, r = lane - gl * R;
    const int64_t j = wave * GPW + gl;                                  // the group, relative to g0
    const bool live = gl < GPW && j < a.n;
    const int64_t g = a.g0 + (live ? j : 0);
    const int64_t idx = g * R + r;
    const uint32_t gid = (uint32_t)(p.g0 + g);
    bool sel = false;
    if (live) {
        if (a.mask) {
            sel = (a.mask[j] >> r) & 1u;
        } else if (a.ppm) {
            const u32x4 w = draw(p, a.t, gid, RAFT_RNG_RESTART, (uint32_t)(r >> 2));
            sel = hit32(word_of(w, r & 3), a.ppm);
        }
    }
    const uint64_t bal = __ballot(sel);
    if (bal == 0) return;                                               // wave-uniform: no state is read
    const bool amnesia = a.flags & RAFT_RESTART_AMNESIA;                // uniform
    const bool replay = a.flags & (RAFT_RESTART_AMNESIA | RAFT_RESTART_REPLAY);
    // this lane's group: which of its replicas restart (0 on a dead lane)
    const uint32_t gmask = live ? (uint32_t)(bal >> (gl * R)) & GROUP_BITS : 0u;

    uint32_t dropped = 0;
    bool was_leader = false;
    if (sel) {
        const int4 q0 = *quad(p, 0, idx);
        const int4 q1 = *quad(p, 1, idx);
        was_leader = q0.z == RAFT_LEADER;
        const u32x4 w = draw(p, a.t, gid, RAFT_RNG_TIMER, (uint32_t)(r >> 2));
        const int32_t elec = scale_range(word_of(w, r & 3), p.emin, p.emax);
        if (amnesia) {
            dropped = (uint32_t)q1.x;
            *quad(p, 0, idx) = make_int4(0, -1, RAFT_FOLLOWER, (int32_t)FL_ARMED);
            *quad(p, 1, idx) = make_int4(0, 0, 0, elec);                // lastIndex 0: an empty tail cache
            *quad(p, 2, idx) = make_int4(0, 0, 0, 0);
        } else {
            const int4 q2 = *quad(p, 2, idx);
            *quad(p, 0, idx) = make_int4(q0.x, q0.y, RAFT_FOLLOWER, (int32_t)FL_ARMED);
            *quad(p, 1, idx) = make_int4(q1.x, q1.y, q1.z, elec);
            *quad(p, 2, idx) = make_int4(0, q2.y, q2.z, 0);             // commitIndex, phaseMs; t2, c1 stay
        }
        p.st[fidx(p, RAFT_F_RETRY_MS, idx)] = 0;
        if (replay) {
            a.applied[idx] = 0;
            if (a.heads) a.heads[idx] = make_int4(0, 0, 0, 0);
        }
    }
    if (gmask) {
        // rows [s][*] of the restarted s, at this lane's column: spill[(g * R + d) * R + s]
#pragma unroll
        for (int s = 0; s < R; ++s)
            if ((gmask >> s) & 1u) {
                p.spill[idx * R + s] = 0;
                p.spill[p.GR * R + idx * R + s] = 0;
            }
        if (r == 0) {                                                   // the group's words
            const int32_t s0 = p.gx[GX_S0 * p.G + g];
            if (s0 >= 0 && ((gmask >> s0) & 1u)) p.gx[GX_S0 * p.G + g] = -1;
            if (a.down_steps > 0) p.gx[GX_ISO * p.G + g] = a.down_steps << 8 | (__ffs(gmask) - 1);
        }
    }
    // the machine's registers of the selected replicas: word q of popc(bal) << logS,
    // 64 a pass; word q belongs to the (q >> logS)-th selected lane
    if (replay && a.heads) {
        const uint32_t words = (uint32_t)__popcll(bal) << a.logS;
        const uint32_t S = 1u << a.logS;
        for (uint32_t q0 = 0; q0 < words; q0 += 64) {                   // wave-uniform trip count
            const uint32_t q = q0 + lane;
            const uint32_t k = q >> a.logS;
            int pos = 0;                        // the k-th set bit of bal: the largest pos with popc(bal below pos) <= k
#pragma unroll
            for (int step = 32; step > 0; step >>= 1) {
                const int c = __popcll(bal & ((1ull << (pos + step)) - 1ull));
                pos = (uint32_t)c <= k ? pos + step : pos;
            }
            const int64_t oi = (int64_t)__shfl((unsigned long long)idx, pos, 64);
            if (q < words) a.regs[oi * S + (q & (S - 1u))] = 0u;
        }
    }
    // the totals
    const uint64_t lead = __ballot(was_leader);
    const uint32_t wd = wave_sum(dropped);                              // 64 lastIndex values of < 2^23 each
    if (lane == 0) {
        unsigned long long* line = stripe_of(a.hdr, wave);
        atomicAdd(line + HDR_RESTARTED, (unsigned long long)__popcll(bal));   // (bal != 0: the wave selected something)
        tally_ballot(line, HDR_LEADERS, lead);
        tally(line, HDR_DROPPED, wd);
    }
}

template <int R> struct RestartL {
    static void run(raft_engine* e, const RestartArgs& a) {
        const int64_t waves = (a.n + (64 / R) - 1) / (64 / R);
        const unsigned grid = (unsigned)((waves + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK);
        restart_kernel<R><<<grid, BLOCK, 0, e->stream>>>(e->dp, a);
    }
};

enum { SEL_HOST = 0, SEL_DEV = 1, SEL_RANDOM = 2 };

int restart(raft_engine* e, int64_t g0, int64_t n, int how, const uint8_t* mask, uint32_t ppm, int32_t flags,
            int32_t down_steps, raft_restart_info* info) {
    if (!e) return raft_internal_fail(RAFT_EINVAL, "null engine");
    if (!info) return raft_internal_fail(RAFT_EINVAL, "null info");
    *info = raft_restart_info{0, 0, 0, 0};
    if (flags & ~(RAFT_RESTART_AMNESIA | RAFT_RESTART_REPLAY))
        return raft_internal_fail(RAFT_EINVAL, "unknown restart flag bits");
    if (down_steps < 0 || down_steps > MAX_DOWN_STEPS)
        return raft_internal_fail(RAFT_EINVAL, "down_steps must be in 0..2^23-1");
    if (int rc = check_groups(e, g0, n)) return rc;
    if (n == 0) return RAFT_OK;
    if (how != SEL_RANDOM && !mask) return raft_internal_fail(RAFT_EINVAL, "null mask");
    HIP_TRY(hipSetDevice(e->device));
    e->fork_needed = true;                           // later step launches wait for the restart
    // staging: the header, then the device copy of a host mask
    if (int rc = raft_internal_grow_dev(e, &e->aux, &e->aux_bytes, Totals::BYTES + (how == SEL_HOST ? (size_t)n : 0)))
        return rc;
    Totals tot;
    if (int rc = tot.zero(e, e->aux)) return rc;
    if (how == SEL_HOST) {
        HIP_TRY(hipMemcpyAsync(e->aux + Totals::BYTES, mask, (size_t)n, hipMemcpyHostToDevice, e->stream));
        mask = (const uint8_t*)(e->aux + Totals::BYTES);
    }
    RestartArgs a{};
    a.g0 = g0;
    a.n = n;
    a.mask = how == SEL_RANDOM ? nullptr : mask;
    a.ppm = ppm;
    a.t = (uint32_t)e->t;
    a.flags = flags;
    a.down_steps = down_steps;
    a.applied = e->applied;
    if (e->sm) {
        a.heads = sm_heads_of(e);
        a.regs = sm_regs_of(e);
        a.logS = log2_slots(e);
    }
    a.hdr = tot.dev;
    by_R<RestartL>(e->p.R, e, a);
    HIP_TRY(hipGetLastError());
    if (int rc = tot.fetch(e)) return rc;
    info->restarted = (int64_t)tot.w[HDR_RESTARTED];
    info->leaders = (int64_t)tot.w[HDR_LEADERS];
    info->entries_dropped = (int64_t)tot.w[HDR_DROPPED];
    if (down_steps > 0 && info->restarted > 0) e->iso_written = true;   // an isolation word: NET_ISO kernels from now on
    return RAFT_OK;
}

}  // namespace

extern "C" {

int raft_engine_restart(raft_engine* e, int64_t g0, int64_t n, const uint8_t* mask_host, int32_t flags,
                        int32_t down_steps, raft_restart_info* info) {
    return restart(e, g0, n, SEL_HOST, mask_host, 0, flags, down_steps, info);
}

int raft_engine_restart_dev(raft_engine* e, int64_t g0, int64_t n, const uint8_t* mask_dev, int32_t flags,
                            int32_t down_steps, raft_restart_info* info) {
    return restart(e, g0, n, SEL_DEV, mask_dev, 0, flags, down_steps, info);
}

int raft_engine_restart_random(raft_engine* e, int64_t g0, int64_t n, uint32_t ppm, int32_t flags,
                               int32_t down_steps, raft_restart_info* info) {
    return restart(e, g0, n, SEL_RANDOM, nullptr, ppm, flags, down_steps, info);
}

}  // extern "C"
