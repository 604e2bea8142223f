// svx_replay.hip — "which haplotype do these edits spell, and do two such haplotypes agree?" for a batch of reference
// windows with lists of small edits on gfx950 (svx_variant_replay, include/svx.h).
//
// The definition is the loop in include/svx.h: a job is a window of the pool and a list of edits (start, ref_len, alt); its
// string is the window with every edit's reference bytes replaced by its alternative bytes; a pair of jobs is equal when
// both strings exist and are the same.
//
// Count, scan, emit, and output BYTES are dealt out, not jobs: a job of 10^5 bases and 10^6 jobs of 60 bases load the
// device alike.  With A(e) / R(e) the sums of alt_len / ref_len over the edits in front of e, edit e of a good job begins
// in the output at   job_off[j] + ed_start[e] + (A(e) - A(first)) - (R(e) - R(first)),   which rises with e: a lane finds
// the edit of its first byte by one upper bound among them and walks forward.
//
// One scan carries four sums in a pair of 64-bit words (Use; svx_lift_exclusive scans such pairs):
//     .ref = alt bytes (low 32)  | edits out of order (high 32)       .qry = edits not inside (low 32) | ref bytes (high 32)
// The low halves cannot carry: the alt bytes of a call are below 2^32 (the entry's bound) and so is the number of edits.
// The high halves wrap, and a difference of two prefixes is still exact modulo 2^32 — the edits of one job are fewer, and
// the ref bytes are only used where the job is good, where they are at most win_len.
//
// Launches, nothing handed between workgroups inside one:
//   k_replay_edit_sums   a workgroup per kScanChunk edits: each edit's job (upper bound among ed_first) and the chunk's Use;
//   k_lift_chunks        exclusive scan of the chunk sums (svx_lift_exclusive);
//   k_replay_edit_pre    the chunk again: the Use in front of every edit, and one entry more: the total;
//   k_replay_jobs        a lane per job: status, out_len, its offset inside its workgroup, the workgroup's bytes;
//   k_lift_chunks        exclusive scan of those, one entry more than workgroups: the total;
//   k_replay_bases       job_off = offset inside the workgroup + the workgroup's base, n_jobs + 1 entries;
//   k_replay_edit_out    every edit's first output byte (job_off[j] for the edits of a job that is not good);
//   k_replay_emit        a workgroup per tile of SVX_REPLAY_TILE output bytes of the whole call, 16 bytes per lane: the
//                        source runs of those bytes, each fetched as five aligned dwords and v_alignbyte so that byte c is
//                        output byte c — the pool offsets have any alignment —, merged under a mask, ONE 16-byte store;
//   k_replay_pairs       a lane per pair: equal[k] = both good and equal lengths, and the bytes to compare (the length, or 0);
//   k_lift_chunks, k_replay_bases   the pairs' offsets among the compared bytes, as for the jobs;
//   k_replay_compare     a workgroup per tile of SVX_REPLAY_TILE compared bytes: both strings' 16 bytes the same way, and a
//                        lane that sees a difference stores 0 to equal[k] — one value from many lanes, no atomic.
// The edit launches are left out for a call without edits, the pair launches for one without pairs.  The emit and compare
// grids come from what the host can bound (windows plus alternative bytes): a tile behind the device's total returns.
// Every word of the scratch that a launch reads was written by this call before: the sums and bases, the prefixes, the
// offsets, the 16 bytes in front of the staged pool and of the strings (memset), the 32 behind the pool (memset) and the 32
// behind the strings (the lane of the last 16 bytes writes them).
#include "svx_internal.h"
#include "svx_scan_dev.h"

namespace {

constexpr int kThreads = kScanThreads;
constexpr int kPer = kScanPer;
constexpr int kBytes = SVX_REPLAY_TILE / kThreads;  // output bytes of one lane
static_assert(kBytes == 16 && kBytes * kThreads == SVX_REPLAY_TILE, "sixteen bytes per lane: one 16-byte store");
constexpr uint64_t kMaxBytes = SVX_REPLAY_MAX_BYTES;  // windows plus alternative bytes of one call
constexpr uint64_t kMaxTiles = 0x7FFFFFFFull;         // gridDim.x
constexpr size_t kPadFront = 16, kPadBack = 32;       // what the 16-byte loads may touch in front of and behind a range

using Use = svx_use;
struct OpUse {
    __device__ __forceinline__ Use operator()(Use a, Use b) const { return Use{a.ref + b.ref, a.qry + b.qry}; }
};

struct Args {
    const uint8_t* bases;
    const uint64_t* win_off;
    const uint32_t* win_len;
    const uint32_t* ed_first;  // n_jobs + 1
    const uint32_t* ed_start;
    const uint32_t* ed_ref_len;
    const uint64_t* ed_alt_off;
    const uint32_t* ed_alt_len;
    const uint32_t* pair_a;
    const uint32_t* pair_b;
    uint32_t n_jobs, n_edits, n_pairs;
    uint32_t* ed_job;    // n_edits
    Use* chunk_sum;      // chunks of edits + 1
    Use* chunk_base;
    Use* pre;            // n_edits + 1
    uint64_t* ed_out;    // n_edits
    Use* group_sum;      // workgroups of jobs + 1
    Use* group_base;
    uint64_t* job_off;   // n_jobs + 1
    uint32_t* out_off;   // n_jobs + 1: job_off as the caller receives it
    Use* pgroup_sum;     // workgroups of pairs + 1
    Use* pgroup_base;
    uint64_t* pair_off;  // n_pairs + 1
    uint32_t* out_len;
    uint8_t* status;
    uint8_t* equal;
    uint8_t* out;        // the strings, 16 bytes behind their slot's start
};

// the 16 bytes at p (any alignment) as four dwords, little endian: five aligned dwords, v_alignbyte
__device__ __forceinline__ void load16(const uint8_t* __restrict__ p, uint32_t* v) {
    const uint32_t sh = (uint32_t)((uintptr_t)p & 3u);
    const uint32_t* __restrict__ w = reinterpret_cast<const uint32_t*>((uintptr_t)p & ~(uintptr_t)3);
    uint32_t x[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) x[k] = w[k];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = __builtin_amdgcn_alignbyte(x[k + 1], x[k], sh);
}
// the bytes [c0, c1) of dword d of a lane's 16, as a mask (0: none of them)
__device__ __forceinline__ uint32_t mask_of(int d, int c0, int c1) {
    const int lo = c0 - 4 * d > 0 ? c0 - 4 * d : 0, hi = c1 - 4 * d < 4 ? c1 - 4 * d : 4;
    if (hi <= lo) return 0u;
    return (hi == 4 ? 0xFFFFFFFFu : (1u << (8 * hi)) - 1u) & ~((1u << (8 * lo)) - 1u);
}

// what edit e of job j adds to the four sums
__device__ __forceinline__ Use use_of(const Args& g, uint64_t e, uint32_t j) {
    const uint64_t s = g.ed_start[e], r = g.ed_ref_len[e];
    bool out_of_order = false;
    if (e != g.ed_first[j]) {
        const uint64_t ps = g.ed_start[e - 1];
        out_of_order = s < ps + g.ed_ref_len[e - 1] || s <= ps;
    }
    const bool not_inside = s + r > g.win_len[j];
    return Use{(uint64_t)g.ed_alt_len[e] | (uint64_t)out_of_order << 32, (uint64_t)not_inside | r << 32};
}

// the jobs of a lane's kPer consecutive edits from `first` on and their inclusive sums (edits at or behind n_edits: nothing)
template <bool FIND>
__device__ __forceinline__ void load_uses(const Args& g, uint64_t first, Use* v) {
    if (FIND) {
        // the chunk's jobs: ed_first[jlo] <= its first edit, ed_first[jhi] <= its last one
        const uint64_t c0 = (uint64_t)blockIdx.x * kScanChunk;
        const uint64_t c1 = min64(c0 + kScanChunk, g.n_edits) - 1;
        const uint64_t jlo = upper_bound(g.ed_first, 0, (uint64_t)g.n_jobs + 1, c0) - 1;
        const uint64_t jhi = upper_bound(g.ed_first, jlo, (uint64_t)g.n_jobs + 1, c1) - 1;
#pragma unroll
        for (int k = 0; k < kPer; ++k)
            if (first + k < g.n_edits) g.ed_job[first + k] = (uint32_t)(upper_bound(g.ed_first, jlo, jhi + 1, first + k) - 1);
    }
#pragma unroll
    for (int k = 0; k < kPer; ++k) v[k] = first + k < g.n_edits ? use_of(g, first + k, g.ed_job[first + k]) : Use{0, 0};
#pragma unroll
    for (int k = 1; k < kPer; ++k) v[k] = OpUse()(v[k - 1], v[k]);
}

__global__ __launch_bounds__(kThreads) void k_replay_edit_sums(const Args g) {
    __shared__ Use s_w[kScanWaves];
    const int tid = (int)threadIdx.x;
    Use v[kPer];
    load_uses<true>(g, (uint64_t)blockIdx.x * kScanChunk + (uint64_t)tid * kPer, v);
    Use total;
    group_before(wave_scan(v[kPer - 1], OpUse()), s_w, tid, OpUse(), &total);
    if (tid == 0) {
        g.chunk_sum[blockIdx.x] = total;
        if (blockIdx.x == 0) g.chunk_sum[gridDim.x] = Use{0, 0};  // its exclusive sum is the total
    }
}

__global__ __launch_bounds__(kThreads) void k_replay_edit_pre(const Args g) {
    __shared__ Use s_w[kScanWaves];
    const int tid = (int)threadIdx.x;
    const uint64_t first = (uint64_t)blockIdx.x * kScanChunk + (uint64_t)tid * kPer;
    Use v[kPer];
    load_uses<false>(g, first, v);
    Use total;
    const Use before = OpUse()(group_before(wave_scan(v[kPer - 1], OpUse()), s_w, tid, OpUse(), &total), g.chunk_base[blockIdx.x]);
#pragma unroll
    for (int k = 0; k < kPer; ++k)
        if (first + k < g.n_edits) g.pre[first + k] = k ? OpUse()(before, v[k - 1]) : before;
    if (blockIdx.x == 0 && tid == 0) g.pre[g.n_edits] = g.chunk_base[gridDim.x];
}

// One length per lane: its offset inside the workgroup to off[i], the workgroup's bytes to sum[blockIdx.x], and a zero
// behind the last workgroup's — the exclusive sum of that entry is the total.  Every lane of the workgroup calls it.
__device__ __forceinline__ void group_offsets(uint64_t len, uint64_t i, uint64_t n, uint64_t* __restrict__ off, Use* __restrict__ sum,
                                              uint64_t* s_w) {
    const int tid = (int)threadIdx.x;
    uint64_t total;
    const uint64_t before = group_before(wave_scan(len, OpAdd()), s_w, tid, OpAdd(), &total);
    if (i < n) off[i] = before;
    if (tid == 0) {
        sum[blockIdx.x] = Use{total, 0};
        if (blockIdx.x == 0) sum[gridDim.x] = Use{0, 0};
    }
}

__global__ __launch_bounds__(kThreads) void k_replay_jobs(const Args g) {
    __shared__ uint64_t s_w[kScanWaves];
    const uint64_t j = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    uint32_t len = 0;
    if (j < g.n_jobs) {
        const uint64_t eb = g.ed_first[j], ee = g.ed_first[j + 1];
        uint64_t d_alt = 0, d_ref = 0;
        if (ee > eb) {
            d_alt = g.pre[ee].ref - g.pre[eb].ref;
            d_ref = g.pre[ee].qry - g.pre[eb].qry;
        }
        const uint8_t st = (uint32_t)(d_alt >> 32) ? 1 : (uint32_t)d_ref ? 2 : 0;
        if (st == 0) len = g.win_len[j] + (uint32_t)d_alt - (uint32_t)(d_ref >> 32);
        g.status[j] = st;
        g.out_len[j] = len;
    }
    group_offsets(len, j, g.n_jobs, g.job_off, g.group_sum, s_w);
}

// off[i] += the base of i's workgroup, and off[n] = the total; off32 (nullable): the same, narrowed
__global__ __launch_bounds__(kThreads) void k_replay_bases(uint64_t* __restrict__ off, uint64_t n, const Use* __restrict__ base,
                                                          uint32_t* __restrict__ off32) {
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i > n) return;
    const uint64_t v = i < n ? off[i] + base[i / kThreads].ref : base[(n + kThreads - 1) / kThreads].ref;
    off[i] = v;
    if (off32) off32[i] = (uint32_t)v;
}

__global__ __launch_bounds__(kThreads) void k_replay_edit_out(const Args g) {
    const uint64_t e = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= g.n_edits) return;
    const uint32_t j = g.ed_job[e];
    uint64_t at = g.job_off[j];
    if (g.status[j] == 0) {
        const uint64_t eb = g.ed_first[j];
        at += (uint64_t)g.ed_start[e] + (uint32_t)(g.pre[e].ref - g.pre[eb].ref) - (uint32_t)((g.pre[e].qry - g.pre[eb].qry) >> 32);
    }
    g.ed_out[e] = at;
}

__global__ __launch_bounds__(kThreads) void k_replay_emit(const Args g) {
    const uint64_t total = g.job_off[g.n_jobs];
    const uint64_t tile0 = (uint64_t)blockIdx.x * SVX_REPLAY_TILE;
    if (tile0 >= total) return;
    const uint64_t o0 = tile0 + (uint64_t)threadIdx.x * kBytes;
    if (o0 >= total) return;
    const uint64_t end = min64(o0 + kBytes, total);
    // the tile's jobs, then the job of this lane's first byte: job_off[j] <= o0 < job_off[j + 1]
    const uint64_t jlo = upper_bound(g.job_off, 0, (uint64_t)g.n_jobs + 1, tile0) - 1;
    const uint64_t jhi = upper_bound(g.job_off, jlo, (uint64_t)g.n_jobs + 1, min64(tile0 + SVX_REPLAY_TILE, total) - 1) - 1;
    uint64_t j = upper_bound(g.job_off, jlo, jhi + 1, o0) - 1;
    uint32_t R[4] = {0, 0, 0, 0};
    uint64_t cur = o0;
    while (cur < end) {
        const uint64_t jb = g.job_off[j], je = g.job_off[j + 1];  // (jb <= cur < je)
        const uint64_t eb = g.ed_first[j], ee = g.ed_first[j + 1];
        const uint64_t stop = min64(je, end);
        uint64_t i = upper_bound(g.ed_out, eb, ee, cur);  // the first edit that begins behind cur
        while (cur < stop) {
            uint64_t src, run_end;
            bool window = true;
            if (i > eb) {
                const uint64_t at = g.ed_out[i - 1], alt_end = at + g.ed_alt_len[i - 1];
                if (cur < alt_end) {  // inside the alternative bytes of edit i - 1
                    src = g.ed_alt_off[i - 1] + (cur - at);
                    run_end = alt_end;
                    window = false;
                } else {  // the window behind edit i - 1
                    src = g.win_off[j] + (uint64_t)g.ed_start[i - 1] + g.ed_ref_len[i - 1] + (cur - alt_end);
                }
            } else {
                src = g.win_off[j] + (cur - jb);
            }
            if (window) run_end = i < ee ? g.ed_out[i] : je;
            const uint64_t seg_end = min64(run_end, stop);
            if (seg_end > cur) {
                const int c0 = (int)(cur - o0), c1 = (int)(seg_end - o0);
                uint32_t Q[4];
                load16(g.bases + src - c0, Q);  // byte c of Q: output byte c of this lane
#pragma unroll
                for (int d = 0; d < 4; ++d) {
                    const uint32_t m = mask_of(d, c0, c1);
                    R[d] = (R[d] & ~m) | (Q[d] & m);
                }
                cur = seg_end;
            }
            if (window && cur == run_end) ++i;  // edit i begins here (its alternative bytes may be none)
        }
        if (cur < end)
            do ++j; while (g.job_off[j + 1] <= cur);  // (cur < total = job_off[n_jobs]: ends inside the list)
    }
    uint4* dst = reinterpret_cast<uint4*>(g.out + o0);
    dst[0] = make_uint4(R[0], R[1], R[2], R[3]);  // (bytes at or behind the total: zeros)
    if (o0 + kBytes >= total) dst[1] = dst[2] = make_uint4(0, 0, 0, 0);  // what the compare's loads may touch behind the strings
}

__global__ __launch_bounds__(kThreads) void k_replay_pairs(const Args g) {
    __shared__ uint64_t s_w[kScanWaves];
    const uint64_t k = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    uint32_t len = 0;
    if (k < g.n_pairs) {
        const uint32_t a = g.pair_a[k], b = g.pair_b[k];
        const bool eq = g.status[a] == 0 && g.status[b] == 0 && g.out_len[a] == g.out_len[b];
        g.equal[k] = eq ? 1 : 0;
        if (eq) len = g.out_len[a];
    }
    group_offsets(len, k, g.n_pairs, g.pair_off, g.pgroup_sum, s_w);
}

__global__ __launch_bounds__(kThreads) void k_replay_compare(const Args g) {
    const uint64_t total = g.pair_off[g.n_pairs];
    const uint64_t tile0 = (uint64_t)blockIdx.x * SVX_REPLAY_TILE;
    if (tile0 >= total) return;
    const uint64_t o0 = tile0 + (uint64_t)threadIdx.x * kBytes;
    if (o0 >= total) return;
    const uint64_t end = min64(o0 + kBytes, total);
    const uint64_t klo = upper_bound(g.pair_off, 0, (uint64_t)g.n_pairs + 1, tile0) - 1;
    const uint64_t khi = upper_bound(g.pair_off, klo, (uint64_t)g.n_pairs + 1, min64(tile0 + SVX_REPLAY_TILE, total) - 1) - 1;
    uint64_t k = upper_bound(g.pair_off, klo, khi + 1, o0) - 1;
    uint64_t cur = o0;
    while (cur < end) {
        const uint64_t kb = g.pair_off[k];  // (kb <= cur < pair_off[k + 1])
        const uint64_t seg_end = min64(g.pair_off[k + 1], end);
        const int c0 = (int)(cur - o0), c1 = (int)(seg_end - o0);
        uint32_t A[4], B[4];
        load16(g.out + g.job_off[g.pair_a[k]] + (cur - kb) - c0, A);
        load16(g.out + g.job_off[g.pair_b[k]] + (cur - kb) - c0, B);
        uint32_t x = 0;
#pragma unroll
        for (int d = 0; d < 4; ++d) x |= (A[d] ^ B[d]) & mask_of(d, c0, c1);
        if (x) g.equal[k] = 0;
        cur = seg_end;
        if (cur < end)
            do ++k; while (g.pair_off[k + 1] <= cur);
    }
}

}  // namespace

extern "C" int svx_variant_replay(svx_ctx* ctx, const uint8_t* bases, uint64_t n_bases, const uint64_t* win_off, const uint32_t* win_len,
                                  const uint32_t* ed_first, uint32_t n_jobs, const uint32_t* ed_start, const uint32_t* ed_ref_len,
                                  const uint64_t* ed_alt_off, const uint32_t* ed_alt_len, uint32_t n_edits, const uint32_t* pair_a,
                                  const uint32_t* pair_b, uint32_t n_pairs, uint32_t* out_len, uint8_t* status, uint8_t* equal,
                                  uint8_t* out, uint32_t* out_off, uint64_t cap, uint64_t* n_out) {
    const char* who = "svx_variant_replay";
    if (!ctx) return SVX_E_INVALID;
    if (n_out) *n_out = 0;
    if (!ed_first) return SVX_E_INVALID;
    if (n_jobs && (!win_off || !win_len || !out_len || !status)) return SVX_E_INVALID;
    if (n_edits && (!ed_start || !ed_ref_len || !ed_alt_off || !ed_alt_len)) return SVX_E_INVALID;
    if (n_pairs && (!pair_a || !pair_b || !equal)) return SVX_E_INVALID;
    if (n_bases && !bases) return SVX_E_INVALID;
    if (ed_first[0] != 0) {
        SVX_SET_ERR(ctx, "%s: ed_first[0] is %u, not 0", who, ed_first[0]);
        return SVX_E_INVALID;
    }
    for (uint32_t j = 0; j < n_jobs; ++j)
        if (ed_first[j + 1] < ed_first[j]) {
            SVX_SET_ERR(ctx, "%s: ed_first decreases at job %u", who, j);
            return SVX_E_INVALID;
        }
    if (ed_first[n_jobs] != n_edits) {
        SVX_SET_ERR(ctx, "%s: ed_first ends at %u, not at the %u edits", who, ed_first[n_jobs], n_edits);
        return SVX_E_INVALID;
    }
    std::vector<uint64_t> most((size_t)n_jobs);  // most[j]: no string of job j is longer (what bounds a pair's bytes)
    uint64_t bound = 0;
    for (uint32_t j = 0; j < n_jobs; ++j) {
        if (win_off[j] > n_bases || win_len[j] > n_bases - win_off[j]) {
            SVX_SET_ERR(ctx, "%s: the window of job %u ends behind the %llu bases", who, j, (unsigned long long)n_bases);
            return SVX_E_INVALID;
        }
        uint64_t m = win_len[j];
        for (uint32_t e = ed_first[j]; e < ed_first[j + 1]; ++e) {
            if (ed_alt_off[e] > n_bases || ed_alt_len[e] > n_bases - ed_alt_off[e]) {
                SVX_SET_ERR(ctx, "%s: the alternative allele of edit %u (job %u) ends behind the %llu bases", who, e, j,
                            (unsigned long long)n_bases);
                return SVX_E_INVALID;
            }
            m += ed_alt_len[e];
        }
        most[j] = m;
        bound += m;
    }
    uint64_t cmp_bound = 0;
    for (uint32_t k = 0; k < n_pairs; ++k) {
        if (pair_a[k] >= n_jobs || pair_b[k] >= n_jobs) {
            SVX_SET_ERR(ctx, "%s: pair %u names jobs %u and %u of %u", who, k, pair_a[k], pair_b[k], n_jobs);
            return SVX_E_INVALID;
        }
        cmp_bound += most[pair_a[k]] < most[pair_b[k]] ? most[pair_a[k]] : most[pair_b[k]];
    }
    if (n_jobs == 0) {
        if (out_off) out_off[0] = 0;
        return SVX_OK;
    }
    const uint64_t n_tiles = (bound + SVX_REPLAY_TILE - 1) / SVX_REPLAY_TILE, n_ctiles = (cmp_bound + SVX_REPLAY_TILE - 1) / SVX_REPLAY_TILE;
    if (bound > kMaxBytes) {
        SVX_SET_ERR(ctx, "%s: %llu window plus alternative bytes, at most %llu (what bounds the strings: their offsets are 32 bits wide)", who,
                    (unsigned long long)bound, (unsigned long long)kMaxBytes);
        return SVX_E_TOO_LARGE;
    }
    if (n_ctiles > kMaxTiles) {
        SVX_SET_ERR(ctx, "%s: up to %llu bytes to compare in the pairs, at most %llu", who, (unsigned long long)cmp_bound,
                    (unsigned long long)(kMaxTiles * SVX_REPLAY_TILE));
        return SVX_E_TOO_LARGE;
    }
    const uint32_t n_chunks = (uint32_t)(((uint64_t)n_edits + kScanChunk - 1) / kScanChunk);
    const uint32_t n_groups = (uint32_t)(((uint64_t)n_jobs + kThreads - 1) / kThreads);
    const uint32_t n_pgroups = (uint32_t)(((uint64_t)n_pairs + kThreads - 1) / kThreads);
    SVX_HIP(ctx, hipSetDevice(ctx->device));
    uint8_t *d_padded, *d_strings;
    Args g;
    svx_takes st, ws;
    st.add_up(&g.win_off, win_off, n_jobs);
    st.add_up(&g.win_len, win_len, n_jobs);
    st.add_up(&g.ed_first, ed_first, (size_t)n_jobs + 1);
    st.add_up(&g.ed_start, ed_start, n_edits);
    st.add_up(&g.ed_ref_len, ed_ref_len, n_edits);
    st.add_up(&g.ed_alt_off, ed_alt_off, n_edits);
    st.add_up(&g.ed_alt_len, ed_alt_len, n_edits);
    st.add_up(&g.pair_a, pair_a, n_pairs);
    st.add_up(&g.pair_b, pair_b, n_pairs);
    st.add(&d_padded, kPadFront + n_bases + kPadBack);
    st.add(&g.out_len, n_jobs);
    st.add(&g.status, n_jobs);
    st.add(&g.equal, n_pairs);
    st.add(&g.out_off, (size_t)n_jobs + 1);
    ws.add(&g.ed_job, n_edits);
    ws.add(&g.chunk_sum, (size_t)n_chunks + 1);
    ws.add(&g.chunk_base, (size_t)n_chunks + 1);
    ws.add(&g.pre, (size_t)n_edits + 1);
    ws.add(&g.ed_out, n_edits);
    ws.add(&g.group_sum, (size_t)n_groups + 1);
    ws.add(&g.group_base, (size_t)n_groups + 1);
    ws.add(&g.job_off, (size_t)n_jobs + 1);
    ws.add(&g.pgroup_sum, (size_t)n_pgroups + 1);
    ws.add(&g.pgroup_base, (size_t)n_pgroups + 1);
    ws.add(&g.pair_off, (size_t)n_pairs + 1);
    ws.add(&d_strings, kPadFront + n_tiles * SVX_REPLAY_TILE + kPadBack);
    SVX_TRY(svx_stage_lay(ctx, st));
    SVX_TRY(svx_ws_lay(ctx, ws));
    // (the loads never use a padding byte, but they fetch it: written like every other word)
    SVX_HIP(ctx, hipMemsetAsync(d_padded, 0, kPadFront, ctx->stream));
    SVX_TRY(svx_upload(ctx, d_padded + kPadFront, bases, n_bases));
    SVX_HIP(ctx, hipMemsetAsync(d_padded + kPadFront + n_bases, 0, kPadBack, ctx->stream));
    SVX_HIP(ctx, hipMemsetAsync(d_strings, 0, kPadFront, ctx->stream));
    g.bases = d_padded + kPadFront;
    g.out = d_strings + kPadFront;
    g.n_jobs = n_jobs;
    g.n_edits = n_edits;
    g.n_pairs = n_pairs;
    SVX_TRY(svx_timing_begin(ctx));
    if (n_edits) {
        hipLaunchKernelGGL(k_replay_edit_sums, dim3(n_chunks), dim3(kThreads), 0, ctx->stream, g);
        SVX_HIP(ctx, hipGetLastError());
        SVX_TRY(svx_lift_exclusive(ctx, g.chunk_sum, n_chunks + 1, g.chunk_base));
        hipLaunchKernelGGL(k_replay_edit_pre, dim3(n_chunks), dim3(kThreads), 0, ctx->stream, g);
        SVX_HIP(ctx, hipGetLastError());
    }
    hipLaunchKernelGGL(k_replay_jobs, dim3(n_groups), dim3(kThreads), 0, ctx->stream, g);
    SVX_HIP(ctx, hipGetLastError());
    SVX_TRY(svx_lift_exclusive(ctx, g.group_sum, n_groups + 1, g.group_base));
    hipLaunchKernelGGL(k_replay_bases, dim3(n_jobs / kThreads + 1), dim3(kThreads), 0, ctx->stream, g.job_off, (uint64_t)n_jobs,
                       (const Use*)g.group_base, g.out_off);
    SVX_HIP(ctx, hipGetLastError());
    if (n_edits) {
        hipLaunchKernelGGL(k_replay_edit_out, dim3((n_edits + kThreads - 1) / kThreads), dim3(kThreads), 0, ctx->stream, g);
        SVX_HIP(ctx, hipGetLastError());
    }
    SVX_TRY(svx_timing_mark(ctx, 1));
    if (n_tiles) {
        hipLaunchKernelGGL(k_replay_emit, dim3((uint32_t)n_tiles), dim3(kThreads), 0, ctx->stream, g);
        SVX_HIP(ctx, hipGetLastError());
    }
    if (n_pairs) {
        hipLaunchKernelGGL(k_replay_pairs, dim3(n_pgroups), dim3(kThreads), 0, ctx->stream, g);
        SVX_HIP(ctx, hipGetLastError());
        SVX_TRY(svx_lift_exclusive(ctx, g.pgroup_sum, n_pgroups + 1, g.pgroup_base));
        hipLaunchKernelGGL(k_replay_bases, dim3(n_pairs / kThreads + 1), dim3(kThreads), 0, ctx->stream, g.pair_off, (uint64_t)n_pairs,
                           (const Use*)g.pgroup_base, (uint32_t*)nullptr);
        SVX_HIP(ctx, hipGetLastError());
        if (n_ctiles) {
            hipLaunchKernelGGL(k_replay_compare, dim3((uint32_t)n_ctiles), dim3(kThreads), 0, ctx->stream, g);
            SVX_HIP(ctx, hipGetLastError());
        }
    }
    SVX_TRY(svx_timing_mark(ctx, 2));
    SVX_TRY(svx_timing_end(ctx));
    SVX_TRY(svx_download(ctx, out_len, (const uint32_t*)g.out_len, n_jobs));
    SVX_TRY(svx_download(ctx, status, (const uint8_t*)g.status, n_jobs));
    SVX_TRY(svx_download(ctx, equal, (const uint8_t*)g.equal, n_pairs));
    if (out_off) SVX_TRY(svx_download(ctx, out_off, (const uint32_t*)g.out_off, (size_t)n_jobs + 1));
    uint64_t total = 0;
    SVX_TRY(svx_download(ctx, &total, (const uint64_t*)(g.job_off + n_jobs), 1));
    SVX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (n_out) *n_out = total;
    if (!out) return SVX_OK;  // the strings stay in the workspace
    const uint64_t k = total < cap ? total : cap;
    if (k) {
        SVX_TRY(svx_download(ctx, out, (const uint8_t*)g.out, k));
        SVX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    return total > cap ? SVX_E_CAPACITY : SVX_OK;
}
