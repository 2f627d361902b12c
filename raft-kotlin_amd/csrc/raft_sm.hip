// raft_sm.hip — the replicated state machine (include/raft_engine.h
// raft_engine_sm_*): a machine per replica that consumes its replica's
// committed entries in log order, on the device, writing nothing per entry.
//
// Kernels of its own, beside the drain (raft_apply.hip) and the client path
// (raft_client.hip); they read the state words and the log rows the step
// kernel keeps and write only the machine's own allocation (raft_engine::sm:
// a header, the heads, the registers).
//   apply   one kernel.  A wave owns 64 consecutive selected replicas: each
//           lane computes its replica's (lo, hi) by the drain's rules (the
//           committed prefix, the ring skip, the regression rule), a wave-local
//           prefix sum of the counts gives the tile's offsets (no global scan,
//           no host read), and the wave walks the tile's entries 64 at a time:
//           a lane finds the owner of its entry by a binary search over the
//           offsets (shuffles, as the drain's expand pass), so lanes inside one
//           run read consecutive 8-byte log slots and the work is balanced by
//           entry, not by replica.  The hash is polynomial, so a batch folds in
//           parallel: a lane forms x * P^(m-1-p) (p: its position in its
//           owner's part of the batch, m: that part's length), a segmented
//           suffix sum brings each part's total to its first lane, the owner
//           lane fetches it and sets hash = hash * P^m + sum.  The registers
//           live in LDS as 64-bit words (index + 1) << 32 | cmd per (owner,
//           slot), updated with an LDS atomic max: the entry with the highest
//           index wins inside a batch and across batches alike, whatever order
//           the lanes' updates land in, and a zero word means untouched.  Each
//           touched (replica, slot) and each head is stored once, when the
//           tile is done.
//   get     one thread per message: the leader lookup of the client path from
//           the R role words, then one register load and one head load
//   check   one thread per group: its R heads
#include <hip/hip_runtime.h>

#include <string>

#include "raft_ledger.h"

using namespace raft;

namespace {

static_assert(sizeof(raft_sm_info) == 32 && sizeof(raft_sm_head) == 16 && sizeof(raft_sm_value) == 16,
              "record layouts of the C-ABI");

// The header: the totals of an apply (Totals, raft_engine_impl.h), these words of a wave's stripe.  Every
// wave with entries adds to `applied`
constexpr int HDR_APPLIED = 0, HDR_LOST = 1, HDR_REGRESSED = 2;
constexpr uint64_t SM_P = 0xD1342543DE82EF95ull, SM_GOLD = 0x9E3779B97F4A7C15ull;
constexpr int PW_WORDS = 66;                                          // P^0 .. P^64 and a pad word, per wave

__device__ __forceinline__ uint64_t sm_x(int32_t i, uint32_t t, uint32_t c) {
    uint64_t z = ((uint64_t)t << 32 | c) + (uint64_t)(uint32_t)i * SM_GOLD;
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}

// One entry of a 64-entry batch, as its lane holds it: the owner lane k, the
// owner's offset and count in the tile, the entry's log index and (term, cmd)
struct Ent {
    int k;
    uint32_t rk, ck;
    int32_t index;
    uint2 e;
};

// Wave w of the grid owns replicas [64 w, 64 w + 64) of the selection.  LDS per
// wave: the powers P^0 .. P^64, then the 64 x S register words.
// NOOP (raft_engine_sm_set_noop enabled): an entry whose cmd is `noop` counts and
// hashes like any other and writes no register; without it `noop` is unused and
// the code is the plain apply's.
template <int R, bool NOOP>
__global__ __launch_bounds__(BLOCK) void sm_apply_kernel(DevParams p, Sel s, int logS, int4* __restrict__ heads,
                                                         uint32_t* __restrict__ regs, unsigned long long* hdr,
                                                         uint32_t noop) {
    extern __shared__ unsigned long long sm_lds[];
    const int S = 1 << logS;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t j0 = ((int64_t)blockIdx.x * (blockDim.x >> 6) + wv) * 64;
    if (j0 >= s.N) return;                                             // wave-uniform
    unsigned long long* pw = sm_lds + (size_t)wv * (PW_WORDS + 64 * S);
    unsigned long long* win = pw + PW_WORDS;
    const int64_t j = j0 + lane;
    const bool mine = j < s.N;
    const int64_t my_idx = sel_idx<R>(s, mine ? j : s.N - 1);
    const int4 hd = heads[my_idx];
    uint32_t skip = 0, regressed = 0, cnt = 0;
    int32_t lo = hd.x;
    if (mine) {
        const int32_t commit = p.st[fidx(p, RAFT_F_COMMIT, my_idx)];
        const int32_t last = p.st[fidx(p, RAFT_F_LAST, my_idx)];
        const int32_t hi = committed_hi(p, commit, last);
        if (p.W != FLAT_W) {                                           // a ring: entries below the window are gone
            const int32_t wl = max(0, p.st[fidx(p, RAFT_F_PHYS, my_idx)] - p.W);
            if (wl > lo && hi > lo) {
                skip = (uint32_t)(min(wl, hi) - lo);
                lo += (int32_t)skip;
            }
        }
        regressed = hi < lo ? 1u : 0u;                                 // the cursor is monotone: nothing, unchanged
        cnt = hi > lo ? (uint32_t)(hi - lo) : 0u;
    }
    // the tile's offsets: an exclusive prefix sum over the lanes (64 replicas of
    // < 2^23 entries fit 32 bits); a lane without entries shares its successor's
    // offset and the lanes past the last run carry the tile's end, so the search
    // below never picks a lane with no entries
    uint32_t inc = cnt;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t v = __shfl_up(inc, d, 64);
        inc += lane >= d ? v : 0u;
    }
    const uint32_t roff = inc - cnt;
    const uint32_t span = __shfl(inc, 63, 64);
    // the totals: one atomic per wave and word, into the wave's stripe of the header
    const uint32_t ws = wave_sum(skip), wr = wave_sum(regressed);
    if (lane == 0) {
        unsigned long long* line = stripe_of(hdr, j0 >> 6);              // the wave's tile of the selection
        tally(line, HDR_APPLIED, span);
        tally(line, HDR_LOST, ws);
        tally(line, HDR_REGRESSED, wr);
    }
    uint64_t hash = (uint64_t)(uint32_t)hd.z | (uint64_t)(uint32_t)hd.w << 32;
    if (span) {                                                        // wave-uniform
        for (int q = lane; q < 64 * S; q += 64) win[q] = 0ull;
        {   // P^lane by squaring; P^64 is what the squarings end on
            uint64_t r = 1, b = SM_P;
#pragma unroll
            for (int bit = 0; bit < 6; ++bit) {
                r = (lane >> bit & 1) ? r * b : r;
                b *= b;
            }
            pw[lane] = r;
            if (lane == 0) pw[64] = b;
        }
        wave_lds_fence();
        // what an entry needs from its owner, fetched by shuffle: the cursor and (group - the
        // tile's first group, replica) in one word (G < 2^31, at most 64 groups a tile)
        const int32_t g = (int32_t)(my_idx / R);
        const int32_t gw = __shfl(g, 0, 64);
        const int32_t pk = (g - gw) << 3 | (int32_t)(my_idx - (int64_t)g * R);
        constexpr int GPW = 64 / R;
        auto fetch = [&](uint32_t x0) {
            const uint32_t x = x0 + lane;
            Ent t;
            // owner: the last lane k with roff[k] <= x (its count is then > 0)
            t.k = 0;
            t.rk = 0;
#pragma unroll
            for (int step = 32; step > 0; step >>= 1) {
                const uint32_t v = __shfl(roff, t.k + step, 64);
                const bool take = v <= x;
                t.k = take ? t.k + step : t.k;
                t.rk = take ? v : t.rk;
            }
            t.ck = __shfl(cnt, t.k, 64);
            t.index = __shfl(lo, t.k, 64) + (int32_t)(x - t.rk);
            const int32_t opk = __shfl(pk, t.k, 64);
            t.e = make_uint2(0u, 0u);
            if (x < span) {
                // the owner's log row (log_of): compile-time R, so no runtime divide
                const int32_t og = gw + (opk >> 3), orr = opk & 7;
                const int32_t w = og / GPW;
                const uint2* row = p.log + ((int64_t)w * 64 + ((og - w * GPW) * R + orr)) * (int64_t)p.nslots;
                t.e = row[(uint32_t)t.index & p.wmask];                // lo <= index < hi <= log_cap: inside the row
            }
            return t;
        };
        Ent cur = fetch(0);
        for (uint32_t x0 = 0; x0 < span; x0 += 64) {                   // wave-uniform trip count
            const Ent t = cur;
            if (x0 + 64 < span) cur = fetch(x0 + 64);                  // the next batch's loads, under this one's fold
            const uint32_t x = x0 + lane;
            const bool live = x < span;
            // the owner's part of this batch ends at entry seg_hi of the tile: m - 1 - p = seg_hi - 1 - x
            const uint32_t seg_hi = min(t.rk + t.ck, x0 + 64);
            uint64_t v = 0;
            if (live) {
                v = sm_x(t.index, t.e.x, t.e.y) * pw[seg_hi - 1 - x];  // x(i, t, c) * P^(m - 1 - p)
                if (!NOOP || t.e.y != noop)
                    atomicMax(&win[t.k * S + (int)(t.e.y & (uint32_t)(S - 1))],
                              (unsigned long long)((uint64_t)(uint32_t)(t.index + 1) << 32 | t.e.y));
            }
            // segmented suffix sum: owners ascend with the lane, so "same owner d lanes on"
            // means the same part; the lanes past the last entry form a part of zeros
            const int kk = live ? t.k : 64;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const uint64_t o = __shfl_down((unsigned long long)v, d, 64);
                const int ko = __shfl_down(kk, d, 64);
                v += (lane + d < 64 && ko == kk) ? o : 0ull;
            }
            // the owner lane takes its part's sum from the part's first lane
            const uint32_t my_lo = max(roff, x0), my_hi = min(roff + cnt, x0 + 64);
            const bool part = cnt > 0 && my_hi > my_lo;
            const uint64_t sum = __shfl((unsigned long long)v, part ? (int)(my_lo - x0) : 0, 64);
            if (part) hash = hash * pw[my_hi - my_lo] + sum;           // hash * P^m + sum
        }
        wave_lds_fence();
        // every touched (replica, slot), once: S passes over the 64 x S words
        for (int q = lane; q < 64 * S; q += 64) {
            const int64_t oi = __shfl((unsigned long long)my_idx, q >> logS, 64);
            const unsigned long long w = win[q];
            if (w) regs[oi * S + (q & (S - 1))] = (uint32_t)w;
        }
    }
    // the head, once per replica that moved
    if (mine && (cnt || skip))
        heads[my_idx] = make_int4(lo + (int32_t)cnt, hd.y + (int32_t)skip, (int32_t)(uint32_t)hash,
                                  (int32_t)(uint32_t)(hash >> 32));
}

// the status word of a get (DevWords, raft_engine_impl.h: one stripe), at the head of cli
enum { GW_RANGE = 0, GW_WORDS = 1 };
constexpr size_t GW_BYTES = 256;
using GetStatus = DevWords<unsigned int, 1, GW_WORDS, GW_WORDS, false>;

__global__ __launch_bounds__(BLOCK) void sm_get_kernel(DevParams p, int S, const int4* __restrict__ heads,
                                                       const uint32_t* __restrict__ regs,
                                                       const int64_t* __restrict__ group,
                                                       const int32_t* __restrict__ replica,
                                                       const uint32_t* __restrict__ key, int4* __restrict__ out, int n,
                                                       unsigned int* flags) {
    const int m = blockIdx.x * BLOCK + threadIdx.x;
    if (m >= n) return;
    const int64_t g = group[m];
    int32_t r = replica[m];
    if (g < 0 || g >= p.G || r < -1 || r >= p.R) {
        atomicOr(&flags[GW_RANGE], 1u);
        out[m] = make_int4(0, -1, 0, 0);
        return;
    }
    if (r < 0) r = find_leader(p, g).r;
    int4 v = make_int4(0, -1, 0, 0);                                    // raft_sm_value of a group without a leader
    if (r >= 0) {
        const int64_t idx = g * p.R + r;
        v = make_int4((int32_t)regs[idx * S + (key[m] & (uint32_t)(S - 1))], r, heads[idx].x, quad(p, 2, idx)->x);
    }
    out[m] = v;
}

// State Machine Safety: two replicas that lost nothing, applied equally many
// entries and hold different hashes
__global__ __launch_bounds__(BLOCK) void sm_check_kernel(DevParams p, const int4* __restrict__ heads, int64_t g0,
                                                         int64_t n, uint8_t* flags, unsigned long long* count) {
    const int64_t k = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    bool bad = false;
    if (k < n) {
        const int R = p.R;
        const int4* h = heads + (g0 + k) * R;
        for (int a = 0; a < R; ++a) {
            const int4 x = h[a];
            for (int b = a + 1; b < R; ++b) {
                const int4 y = h[b];
                bad |= x.y == 0 && y.y == 0 && x.x == y.x && (x.z != y.z || x.w != y.w);
            }
        }
        if (flags) flags[k] = bad ? 1 : 0;
    }
    const unsigned long long any = __ballot(bad);
    if ((threadIdx.x & 63) == 0 && any) atomicAdd(count, (unsigned long long)__popcll(any));
}

// waves per workgroup of an apply: the 64 x S register words of every wave within 32 KB of LDS
int apply_waves(int S) { return S <= 16 ? WAVES_PER_BLOCK : S == 32 ? 2 : 1; }

template <int R> struct ApplyL {
    static void run(raft_engine* e, const Sel& s, int logS, unsigned long long* hdr) {
        const int S = 1 << logS, wpb = apply_waves(S);
        const int64_t tiles = (s.N + 63) / 64;
        const unsigned grid = (unsigned)((tiles + wpb - 1) / wpb);
        const size_t lds = (size_t)wpb * (PW_WORDS + 64 * S) * 8;
        if (e->sm_noop_on)
            sm_apply_kernel<R, true><<<grid, wpb * 64, lds, e->stream>>>(e->dp, s, logS, sm_heads_of(e), sm_regs_of(e),
                                                                         hdr, e->sm_noop_cmd);
        else
            sm_apply_kernel<R, false><<<grid, wpb * 64, lds, e->stream>>>(e->dp, s, logS, sm_heads_of(e),
                                                                          sm_regs_of(e), hdr, 0u);
    }
};

}  // namespace

extern "C" {

int raft_engine_sm_configure(raft_engine* e, int32_t slots) {
    if (!e) return raft_internal_fail(RAFT_EINVAL, "null engine");
    if (slots < 0 || slots > 64 || (slots & (slots - 1)))
        return raft_internal_fail(RAFT_EINVAL, "slots must be 0 (free) or a power of two in 1..64");
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (e->sm && slots != e->sm_slots) {
        HIP_TRY(hipFree(e->sm));
        e->sm = nullptr;
        e->sm_bytes = 0;
        e->sm_slots = 0;
    }
    if (slots == 0) return RAFT_OK;
    if (!e->sm) {
        const size_t bytes = Totals::BYTES + al256((size_t)e->dp.GR * 16) + al256((size_t)e->dp.GR * slots * 4);
        if (hipMalloc((void**)&e->sm, bytes) != hipSuccess) {
            e->sm = nullptr;
            return raft_internal_fail(RAFT_ENOMEM, "hipMalloc of " + std::to_string(bytes) +
                                                       " bytes for the state machine failed");
        }
        e->sm_bytes = bytes;
        e->sm_slots = slots;
    }
    HIP_TRY(hipMemsetAsync(e->sm, 0, e->sm_bytes, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return RAFT_OK;
}

int raft_engine_sm_set_noop(raft_engine* e, int enable, uint32_t cmd) {
    if (!e) return raft_internal_fail(RAFT_EINVAL, "null engine");
    e->sm_noop_on = enable != 0;                     // read at the next apply's launch: nothing is enqueued
    e->sm_noop_cmd = enable ? cmd : 0u;
    return RAFT_OK;
}

int raft_engine_sm_apply(raft_engine* e, int64_t g0, int64_t n, int32_t replica, raft_sm_info* info) {
    if (int rc = check_sm(e)) return rc;
    if (!info) return raft_internal_fail(RAFT_EINVAL, "null info");
    if (int rc = check_groups(e, g0, n)) return rc;
    if (replica < -1 || replica >= e->p.R) return raft_internal_fail(RAFT_EINVAL, "replica must be -1 or in 0..R-1");
    *info = raft_sm_info{0, 0, 0, 0};
    if (n == 0) return RAFT_OK;
    HIP_TRY(hipSetDevice(e->device));
    e->fork_needed = true;                           // later step launches wait for these reads of the state and logs
    const Sel s{g0, replica < 0 ? n * e->p.R : n, replica};
    Totals tot;
    if (int rc = tot.zero(e, e->sm)) return rc;
    if (e->sm_timing) HIP_TRY(hipEventRecord(e->ev_sm[0], e->stream));
    by_R<ApplyL>(e->p.R, e, s, log2_slots(e), tot.dev);
    HIP_TRY(hipGetLastError());
    if (e->sm_timing) HIP_TRY(hipEventRecord(e->ev_sm[1], e->stream));
    if (int rc = tot.fetch(e)) return rc;
    info->applied = (int64_t)tot.w[HDR_APPLIED];
    info->lost = (int64_t)tot.w[HDR_LOST];
    info->regressed = (int64_t)tot.w[HDR_REGRESSED];
    if (info->lost > 0)
        return raft_internal_fail(RAFT_EWINDOW, std::to_string(info->lost) +
                                                    " committed entries left the log window unapplied (skipped)");
    return RAFT_OK;
}

// replicas are indexed g * R + r: a range of groups is one contiguous run of heads and one of registers; either
// pointer may be null (that region is skipped), so the shared head's null-buffer refusal does not apply
int raft_engine_sm_read(raft_engine* e, int64_t g0, int64_t n, raft_sm_head* heads, uint32_t* regs) {
    if (int rc = check_sm(e)) return rc;
    if (int rc = check_groups(e, g0, n)) return rc;
    if (n == 0) return RAFT_OK;
    const size_t r0 = (size_t)g0 * e->p.R, rn = (size_t)n * e->p.R, S = (size_t)e->sm_slots;
    return rows_out(e, {{sm_heads_of(e) + r0, heads, rn * 16}, {sm_regs_of(e) + r0 * S, regs, rn * S * 4}});
}

int raft_engine_sm_write(raft_engine* e, int64_t g0, int64_t n, const raft_sm_head* heads, const uint32_t* regs) {
    if (int rc = check_sm(e)) return rc;
    if (int rc = check_groups(e, g0, n)) return rc;
    if (n == 0) return RAFT_OK;
    const size_t r0 = (size_t)g0 * e->p.R, rn = (size_t)n * e->p.R, S = (size_t)e->sm_slots;
    if (heads)
        for (size_t k = 0; k < rn; ++k) {            // an apply reads log slots [applied, hi): keep it inside the row
            if (heads[k].applied < 0 || heads[k].applied > e->p.log_cap)
                return raft_internal_fail(RAFT_EINVAL, "applied must be in 0..log_cap");
            if (heads[k].lost < 0) return raft_internal_fail(RAFT_EINVAL, "lost must be >= 0");
        }
    return rows_in(e, {{sm_heads_of(e) + r0, heads, rn * 16}, {sm_regs_of(e) + r0 * S, regs, rn * S * 4}});
}

int raft_engine_sm_get(raft_engine* e, const int64_t* group, const int32_t* replica, const uint32_t* key,
                       raft_sm_value* out, int64_t n) {
    if (int rc = check_sm(e)) return rc;
    if (int rc = check_args(e, n, !group || !replica || !key || !out)) return rc;
    if (n == 0) return RAFT_OK;
    HIP_TRY(hipSetDevice(e->device));
    e->fork_needed = true;
    const void* src[3] = {group, replica, key};
    const size_t bytes[3] = {(size_t)n * 8, (size_t)n * 4, (size_t)n * 4};
    Staged s;
    if (int rc = stage_in(e, src, bytes, 3, (size_t)n * sizeof(raft_sm_value), s)) return rc;
    if (int rc = raft_internal_grow_dev(e, &e->cli, &e->cli_bytes, GW_BYTES)) return rc;
    GetStatus st;
    if (int rc = st.zero(e, e->cli)) return rc;
    sm_get_kernel<<<grid_of(n), BLOCK, 0, e->stream>>>(
        e->dp, e->sm_slots, sm_heads_of(e), sm_regs_of(e), (const int64_t*)(e->cio + s.off[0]),
        (const int32_t*)(e->cio + s.off[1]), (const uint32_t*)(e->cio + s.off[2]), (int4*)(e->cio + s.out_off), (int)n,
        st.dev);
    HIP_TRY(hipGetLastError());
    if (int rc = stage_out_dma(e, s)) return rc;
    if (int rc = st.fetch(e)) return rc;                                // (waits for the records too)
    if (st.w[GW_RANGE])
        return raft_internal_fail(RAFT_ERANGE, "a read's group or replica is outside the engine; nothing was filled");
    stage_out_copy(e, s, out);
    return RAFT_OK;
}

int raft_engine_sm_check(raft_engine* e, int64_t g0, int64_t n, uint8_t* flags, int64_t* diverged) {
    if (int rc = check_sm(e)) return rc;
    if (int rc = check_groups(e, g0, n)) return rc;
    if (!diverged) return raft_internal_fail(RAFT_EINVAL, "null argument");
    *diverged = 0;
    if (n == 0) return RAFT_OK;
    HIP_TRY(hipSetDevice(e->device));
    if (int rc = raft_internal_grow_dev(e, &e->aux, &e->aux_bytes, 8 + (flags ? (size_t)n : 0))) return rc;
    unsigned long long* cnt = (unsigned long long*)e->aux;
    uint8_t* fl = flags ? (uint8_t*)e->aux + 8 : nullptr;
    unsigned long long h = 0;
    HIP_TRY(hipMemsetAsync(cnt, 0, 8, e->stream));
    sm_check_kernel<<<grid_of(n), BLOCK, 0, e->stream>>>(e->dp, sm_heads_of(e), g0, n, fl, cnt);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&h, cnt, 8, hipMemcpyDeviceToHost, e->stream));
    if (flags) HIP_TRY(hipMemcpyAsync(flags, fl, (size_t)n, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    *diverged = (int64_t)h;
    return RAFT_OK;
}

// Not in the header (scripts/sm_probe.py): while enabled, an apply records an
// event on either side of its kernel; *ms is the last apply's kernel alone.
int raft_internal_sm_timing(raft_engine* e, int enable) {
    if (!e) return raft_internal_fail(RAFT_EINVAL, "null engine");
    HIP_TRY(hipSetDevice(e->device));
    for (hipEvent_t& x : e->ev_sm)
        if (enable && !x) HIP_TRY(hipEventCreate(&x));
    e->sm_timing = enable != 0;
    return RAFT_OK;
}

int raft_internal_sm_kernel_ms(raft_engine* e, double* ms) {
    if (!e || !ms || !e->sm_timing) return raft_internal_fail(RAFT_EINVAL, "state machine timing is off");
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipStreamSynchronize(e->stream));
    float f = 0.f;
    HIP_TRY(hipEventElapsedTime(&f, e->ev_sm[0], e->ev_sm[1]));
    *ms = f;
    return RAFT_OK;
}

}  // extern "C"
