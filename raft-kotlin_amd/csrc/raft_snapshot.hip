// raft_snapshot.hip — snapshot install on the device (include/raft_engine.h
// raft_engine_install_snapshot*): a replica that fell behind its leader gets the
// leader's retained log, its machine and its commit point, in HBM, between two
// step launches.  Raft paper §7; the reference has no counterpart.
//
// One kernel for the two entry points (a host mask, a device mask), placed like
// restart_kernel (raft_fault.hip): a wave holds GPW = 64 / R whole groups, one
// lane per replica, so the leader choice and every per-group fact is a shuffle
// or a slice of a wave ballot, and no group word is touched by an atomic.
//   leader     every live lane reads quad 0 (role, term); the group's newest
//              leader (find_newest_leader's rule: highest term, lowest index
//              among equals) is found by R shuffles.  Its lane reads its
//              machine's head: a gapped leader installs nothing.
//   selection  quad 1 (lastIndex) decides the lag.  A wave that installs
//              nothing adds its counts and returns here.
//   replica    quads 0-2 are written whole from the leader's words; quad 3 is
//              read and written whole (retryMs 0; the primary session's column
//              towards this replica when the leader owns the primary slot).
//   sessions   rows [f][*] of an installed f become zero in spill and f loses
//              the primary slot if it owned it, as in restart_kernel; the
//              leader's words towards f go to the primary slot (L == s0) or to
//              spill.
//   log        balanced by slot, not by replica: an installed lane owns
//              physLen_L - floor slots, the wave takes the exclusive prefix sum
//              of those counts and walks the tile's slots 64 a pass; a lane
//              finds its slot's owner by a binary search over the offsets
//              (sm_apply_kernel's expand pass) and moves one 8-byte slot from
//              the leader's row to the owner's, consecutive lanes of a run at
//              consecutive slots.  The leader is never installed, so no row is
//              both read and written.
//   machine    heads: one 16-byte store per replica; registers: popc(ballot)
//              << logS words by restart_kernel's k-th-set-bit scheme, read from
//              the leader's.
//   totals     per wave, one atomic per nonzero word into the wave's stripe
//              (DevWords, raft_engine_impl.h); the host sums it.
#include <hip/hip_runtime.h>

#include <string>

#include "raft_stream.h"

using namespace raft;

namespace {

static_assert(sizeof(raft_install_info) == 64, "record layout of the C-ABI");

// the totals of an install: Totals' header (raft_engine_impl.h) with five words of a stripe's line in use
constexpr int HDR_INSTALLED = 0, HDR_SLOTS = 1, HDR_NO_LEADER = 2, HDR_GAPPED = 3, HDR_AHEAD = 4;
using InstallTotals = DevWords<unsigned long long, HDR_STRIPES, HDR_LINE, 5, true>;
static_assert(InstallTotals::BYTES == Totals::BYTES, "the same header");

struct InstallArgs {
    int64_t g0, n;                 // groups [g0, g0 + n)
    const uint8_t* mask;           // [n] device bytes, or nullptr: every replica is eligible
    int32_t min_lag;
    uint32_t t;                    // the engine's step index (Philox c0 of the election draw)
    int4* heads;                   // the machine's heads [G * R]
    uint32_t* regs;                // its registers [G * R][1 << logS]
    int32_t logS;
    unsigned long long* hdr;
};

template <int R>
__global__ __launch_bounds__(BLOCK) void install_kernel(DevParams p, InstallArgs a) {
    constexpr int GPW = 64 / R;
    constexpr uint32_t GROUP_BITS = (1u << R) - 1u;
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * WAVES_PER_BLOCK + (threadIdx.x >> 6);
    const int gl = lane / R, r = lane - gl * R;
    const int64_t j = wave * GPW + gl;                                  // the group, relative to g0
    const bool live = gl < GPW && j < a.n;
    const int64_t g = a.g0 + (live ? j : 0);
    const int64_t idx = g * R + r;
    const int base = live ? gl * R : 0;                                 // lane of this group's replica 0
    const bool elig = live && (a.mask ? (a.mask[j] >> r) & 1u : true);

    // ---- the group's newest leader
    const int4 q0 = live ? *quad(p, 0, idx) : make_int4(0, -1, RAFT_FOLLOWER, 0);
    const int4 q1 = live ? *quad(p, 1, idx) : make_int4(0, 0, 0, 0);
    int32_t L = -1, T = 0;
#pragma unroll
    for (int s = 0; s < R; ++s) {                                       // ascending: of equal terms the lowest id stays
        const int32_t role_s = __shfl(q0.z, base + s, 64), term_s = __shfl(q0.x, base + s, 64);
        const bool take = role_s == RAFT_LEADER && (L < 0 || term_s > T);
        L = take ? s : L;
        T = take ? term_s : T;
    }
    L = live ? L : -1;
    const int ll = base + max(L, 0);                                    // the leader's lane
    const bool is_lead = live && r == L;
    int4 hd = make_int4(0, 0, 0, 0);
    if (is_lead) hd = a.heads[idx];
    const int32_t lastL = __shfl(q1.x, ll, 64);
    const int32_t physL = min(max(__shfl(q1.y, ll, 64), 0), p.cap);     // write_state keeps physLen in 0..log_cap
    const bool gapped = __shfl(hd.y, ll, 64) != 0;
    const bool cand = elig && L >= 0 && !gapped && r != L;
    const bool ahead = cand && q0.x > T;
    const bool inst = cand && q0.x <= T && lastL - q1.x >= a.min_lag;
    const uint64_t bal = __ballot(inst);

    // ---- the totals but the slots; a wave that installs nothing is done
    const uint64_t b_nl = __ballot(live && r == 0 && L < 0), b_gp = __ballot(live && r == 0 && L >= 0 && gapped);
    const uint64_t b_ah = __ballot(ahead);
    unsigned long long* line = stripe_of(a.hdr, wave);
    if (lane == 0) {
        tally_ballot(line, HDR_INSTALLED, bal);
        tally_ballot(line, HDR_NO_LEADER, b_nl);
        tally_ballot(line, HDR_GAPPED, b_gp);
        tally_ballot(line, HDR_AHEAD, b_ah);
    }
    if (bal == 0) return;                                               // wave-uniform
    // this lane's group: which of its replicas are installed (0 on a dead lane)
    const uint32_t gmask = live ? (uint32_t)(bal >> (gl * R)) & GROUP_BITS : 0u;

    // ---- the leader's other words, by shuffle from its lane
    int4 q2 = make_int4(0, 0, 0, 0);
    if (is_lead && gmask) q2 = *quad(p, 2, idx);
    const int32_t t1L = __shfl(q1.z, ll, 64), commitL = __shfl(q2.x, ll, 64), t2L = __shfl(q2.y, ll, 64);
    const int32_t c1L = __shfl(q2.z, ll, 64);
    const int4 hdL = make_int4(__shfl(hd.x, ll, 64), __shfl(hd.y, ll, 64), __shfl(hd.z, ll, 64), __shfl(hd.w, ll, 64));
    const int32_t floorL = max(0, physL - p.W);                         // FLAT_W on a flat log: 0
    int32_t s0 = -1;
    if (gmask) s0 = p.gx[GX_S0 * p.G + g];

    // ---- the installed replicas' scalars, the machine's head, the leader's session towards them
    if (inst) {
        const uint32_t gid = (uint32_t)(p.g0 + g);
        const u32x4 w = draw(p, a.t, gid, RAFT_RNG_TIMER, (uint32_t)(r >> 2));
        const int32_t elec = scale_range(word_of(w, r & 3), p.emin, p.emax);
        const int4 q3 = *quad(p, 3, idx);
        const bool prim = s0 == L;                                      // the leader owns the primary slot
        *quad(p, 0, idx) = make_int4(T, q0.x == T ? q0.y : -1, RAFT_FOLLOWER, (int32_t)FL_ARMED);
        *quad(p, 1, idx) = make_int4(lastL, physL, t1L, elec);
        *quad(p, 2, idx) = make_int4(committed_hi(p, commitL, lastL), t2L, c1L, 0);
        *quad(p, 3, idx) = make_int4(0, prim ? lastL + 1 : q3.y, prim ? lastL : q3.z, q3.w);
        if (!prim) {
            p.spill[idx * R + L] = lastL + 1;
            p.spill[p.GR * R + idx * R + L] = lastL;
        }
        a.heads[idx] = hdL;
    }
    if (gmask) {
        // rows [s][*] of the installed s, at this lane's column: spill[(g * R + d) * R + s]; s != L
#pragma unroll
        for (int s = 0; s < R; ++s)
            if ((gmask >> s) & 1u) {
                p.spill[idx * R + s] = 0;
                p.spill[p.GR * R + idx * R + s] = 0;
            }
        if (r == 0 && s0 >= 0 && ((gmask >> s0) & 1u)) p.gx[GX_S0 * p.G + g] = -1;
    }

    // ---- the log: slot x of the tile belongs to the last lane k with roff[k] <= x
    const uint32_t cnt = inst ? (uint32_t)(physL - floorL) : 0u;       // <= min(W, log_cap) = the row's slots
    uint32_t inc = cnt;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t v = __shfl_up(inc, d, 64);
        inc += lane >= d ? v : 0u;
    }
    const uint32_t roff = inc - cnt;                                    // a lane without slots shares its successor's
    const uint32_t span = __shfl(inc, 63, 64);                          // 64 rows of < 2^23 slots fit 32 bits
    if (lane == 0 && span) atomicAdd(line + HDR_SLOTS, (unsigned long long)span);
    // the owner's row in p.log (log_of, with a compile-time R) and, packed, its first slot and the way to the leader's row
    const int64_t wv = g / GPW;
    const int64_t row = (wv * 64 + ((g - wv * GPW) * R + r)) * (int64_t)p.nslots;
    const int32_t pk = floorL << 4 | (L - r + 8);                       // floor < 2^23; L - r in -7..7
    for (uint32_t x0 = 0; x0 < span; x0 += 64) {                        // wave-uniform trip count
        const uint32_t x = x0 + lane;
        int k = 0;
        uint32_t rk = 0;
#pragma unroll
        for (int step = 32; step > 0; step >>= 1) {
            const uint32_t v = __shfl(roff, k + step, 64);
            const bool take = v <= x;
            k = take ? k + step : k;
            rk = take ? v : rk;
        }
        const int64_t orow = (int64_t)__shfl((unsigned long long)row, k, 64);
        const int32_t opk = __shfl(pk, k, 64);
        if (x < span) {
            const uint32_t slot = (uint32_t)((opk >> 4) + (int32_t)(x - rk)) & p.wmask;   // floor <= index < physLen_L
            const int64_t lrow = orow + (int64_t)((opk & 15) - 8) * p.nslots;
            p.log[orow + slot] = p.log[lrow + slot];
        }
    }

    // ---- the machine's registers of the installed replicas: word q of popc(bal) << logS, 64 a pass; word q
    // belongs to the (q >> logS)-th installed lane and comes from its group's leader
    {
        const uint32_t words = (uint32_t)__popcll(bal) << a.logS;
        const uint32_t S = 1u << a.logS;
        const int64_t lidx = idx - r + max(L, 0);
        for (uint32_t w0 = 0; w0 < words; w0 += 64) {                   // wave-uniform trip count
            const uint32_t q = w0 + lane;
            const uint32_t k = q >> a.logS;
            int pos = 0;                        // the k-th set bit of bal: the largest pos with popc(bal below pos) <= k
#pragma unroll
            for (int step = 32; step > 0; step >>= 1) {
                const int c = __popcll(bal & ((1ull << (pos + step)) - 1ull));
                pos = (uint32_t)c <= k ? pos + step : pos;
            }
            const int64_t oi = (int64_t)__shfl((unsigned long long)idx, pos, 64);
            const int64_t li = (int64_t)__shfl((unsigned long long)lidx, pos, 64);
            if (q < words) a.regs[oi * S + (q & (S - 1u))] = a.regs[li * S + (q & (S - 1u))];
        }
    }
}

template <int R> struct InstallL {
    static void run(raft_engine* e, const InstallArgs& a) {
        const int64_t waves = (a.n + (64 / R) - 1) / (64 / R);
        const unsigned grid = (unsigned)((waves + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK);
        install_kernel<R><<<grid, BLOCK, 0, e->stream>>>(e->dp, a);
    }
};

int install(raft_engine* e, int64_t g0, int64_t n, bool host_mask, const uint8_t* mask, int32_t min_lag,
            raft_install_info* info) {
    if (!e) return raft_internal_fail(RAFT_EINVAL, "null engine");
    if (!info) return raft_internal_fail(RAFT_EINVAL, "null info");
    *info = raft_install_info{};
    if (int rc = check_sm(e)) return rc;
    if (min_lag < 0) return raft_internal_fail(RAFT_EINVAL, "min_lag must not be negative");
    if (int rc = check_groups(e, g0, n)) return rc;
    if (n == 0) return RAFT_OK;
    HIP_TRY(hipSetDevice(e->device));
    e->fork_needed = true;                           // later step launches wait for the install
    // staging: the header, then the device copy of a host mask
    const bool stage = host_mask && mask;
    if (int rc = raft_internal_grow_dev(e, &e->aux, &e->aux_bytes, InstallTotals::BYTES + (stage ? (size_t)n : 0)))
        return rc;
    InstallTotals tot;
    if (int rc = tot.zero(e, e->aux)) return rc;
    if (stage) {
        HIP_TRY(hipMemcpyAsync(e->aux + InstallTotals::BYTES, mask, (size_t)n, hipMemcpyHostToDevice, e->stream));
        mask = (const uint8_t*)(e->aux + InstallTotals::BYTES);
    }
    InstallArgs a{};
    a.g0 = g0;
    a.n = n;
    a.mask = mask;
    a.min_lag = min_lag;
    a.t = (uint32_t)e->t;
    a.heads = sm_heads_of(e);
    a.regs = sm_regs_of(e);
    a.logS = log2_slots(e);
    a.hdr = tot.dev;
    by_R<InstallL>(e->p.R, e, a);
    HIP_TRY(hipGetLastError());
    if (int rc = tot.fetch(e)) return rc;
    info->installed = (int64_t)tot.w[HDR_INSTALLED];
    info->slots_copied = (int64_t)tot.w[HDR_SLOTS];
    info->no_leader = (int64_t)tot.w[HDR_NO_LEADER];
    info->leader_gapped = (int64_t)tot.w[HDR_GAPPED];
    info->ahead = (int64_t)tot.w[HDR_AHEAD];
    return RAFT_OK;
}

}  // namespace

extern "C" {

int raft_engine_install_snapshot(raft_engine* e, int64_t g0, int64_t n, const uint8_t* mask_host, int32_t min_lag,
                                 raft_install_info* info) {
    return install(e, g0, n, true, mask_host, min_lag, info);
}

int raft_engine_install_snapshot_dev(raft_engine* e, int64_t g0, int64_t n, const uint8_t* mask_dev, int32_t min_lag,
                                     raft_install_info* info) {
    return install(e, g0, n, false, mask_dev, min_lag, info);
}

}  // extern "C"
