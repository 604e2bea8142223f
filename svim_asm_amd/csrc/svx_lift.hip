// svx_lift.hip — "where does this reference position lie on the aligned contig?" for a batch of (alignment, position)
// queries against a CIGAR pool on gfx950 (svx_cigar_lift, include/svx.h).
//
// Every op consumes (reference, query) bases by its code alone; with P_ref / P_qry the inclusive prefix sums of both over
// the WHOLE pool, the op of alignment a that covers reference position r is the first op i of the alignment with
//     P_ref[i] > r - ref_start[a] + P_ref[first op of a - 1]
// — it consumes reference (its prefix exceeds its predecessor's), and the query cursor in front of it is P_qry[i - 1]
// less the alignment's base.  So a plain reduce-then-scan over the pool and one binary search per query answer the batch,
// in four launches with nothing handed between workgroups inside one:
//   k_lift_sums    one workgroup per chunk of SVX_LIFT_CHUNK ops: the chunk's (reference, query) sum;
//   k_lift_chunks  ONE workgroup: exclusive prefixes of the chunk sums, the carried scan of svx_scan_dev.h under sum;
//   k_lift_apply   one workgroup per chunk: the ops' consumption again, scanned inside the workgroup on the ladder of
//                  svx_scan_dev.h, plus the chunk's base: P_ref and P_qry, 64 bits each, into the context workspace;
//   k_lift_query   one lane per query: upper bound among the alignment's P_ref, for END one more.
// The prefixes are 64 bits wide: forty alignments of 2^27 reference bases pass 2^32.  Every word of the chunk sums, the
// chunk bases and the prefixes is written before the launch that reads it starts, and only words inside [0, n_ops) and
// [0, n_chunks) are read: nothing depends on what the workspace held (the scratch contract, include/svx.h).
#include "svx_internal.h"
#include "svx_scan_dev.h"

namespace {

constexpr int kThreads = kScanThreads;
constexpr int kPer = kScanPer;
static_assert(SVX_LIFT_CHUNK == kScanChunk, "the public chunk is one workgroup's ops and one pass of the carried scan");
constexpr uint64_t kMaxChunks = 0x7FFFFFFFull;  // gridDim.x

// (reference, query) bases; (0, 0) is the sum's identity
using Use = svx_use;
struct OpUse {
    __device__ __forceinline__ Use operator()(Use a, Use b) const { return Use{a.ref + b.ref, a.qry + b.qry}; }
};
// M D N = X consume reference, M I S = X query (SEQ) bases; H, P and codes above 8 nothing (svx_cigar_stats)
constexpr uint32_t kRefOps = 1u << 0 | 1u << 2 | 1u << 3 | 1u << 7 | 1u << 8;
constexpr uint32_t kQryOps = 1u << 0 | 1u << 1 | 1u << 4 | 1u << 7 | 1u << 8;
__device__ __forceinline__ Use use_of(uint32_t word) {
    const uint32_t op = word & 15u, len = word >> 4;
    return Use{(kRefOps >> op) & 1u ? len : 0u, (kQryOps >> op) & 1u ? len : 0u};
}

// the inclusive sums of a thread's kPer consecutive ops of the chunk at `first` (ops at or behind n_ops: nothing)
__device__ __forceinline__ void load_uses(const uint32_t* __restrict__ cigar, uint64_t first, uint64_t n_ops, Use* v) {
#pragma unroll
    for (int j = 0; j < kPer; ++j) v[j] = first + j < n_ops ? use_of(cigar[first + j]) : Use{0, 0};
#pragma unroll
    for (int j = 1; j < kPer; ++j) v[j] = OpUse()(v[j - 1], v[j]);
}

__global__ __launch_bounds__(kThreads) void k_lift_sums(const uint32_t* __restrict__ cigar, uint64_t n_ops, Use* __restrict__ chunk_sum) {
    __shared__ Use s_w[kScanWaves];
    const int tid = (int)threadIdx.x;
    Use v[kPer];
    load_uses(cigar, (uint64_t)blockIdx.x * SVX_LIFT_CHUNK + (uint64_t)tid * kPer, n_ops, v);
    Use total;
    group_before(wave_scan(v[kPer - 1], OpUse()), s_w, tid, OpUse(), &total);
    if (tid == 0) chunk_sum[blockIdx.x] = total;
}

// chunk_base[c] = chunk_sum[0] + .. + chunk_sum[c - 1]: one workgroup
__global__ __launch_bounds__(kThreads) void k_lift_chunks(const Use* __restrict__ chunk_sum, uint32_t n_chunks, Use* __restrict__ chunk_base) {
    __shared__ Use s_wave[2][kScanWaves];
    carried_scan(0, n_chunks, OpUse(), [=](uint64_t i) { return chunk_sum[i]; }, [=](uint64_t i, Use before, Use) { chunk_base[i] = before; },
                 s_wave);
}

__global__ __launch_bounds__(kThreads) void k_lift_apply(const uint32_t* __restrict__ cigar, uint64_t n_ops, const Use* __restrict__ chunk_base,
                                                         uint64_t* __restrict__ p_ref, uint64_t* __restrict__ p_qry) {
    __shared__ Use s_w[kScanWaves];
    const int tid = (int)threadIdx.x;
    const uint64_t first = (uint64_t)blockIdx.x * SVX_LIFT_CHUNK + (uint64_t)tid * kPer;
    Use v[kPer];
    load_uses(cigar, first, n_ops, v);
    Use total;
    const Use before = OpUse()(group_before(wave_scan(v[kPer - 1], OpUse()), s_w, tid, OpUse(), &total), chunk_base[blockIdx.x]);
#pragma unroll
    for (int j = 0; j < kPer; ++j)
        if (first + j < n_ops) {
            p_ref[first + j] = before.ref + v[j].ref;
            p_qry[first + j] = before.qry + v[j].qry;
        }
}

__global__ __launch_bounds__(kThreads) void k_lift_query(const uint32_t* __restrict__ cigar, const uint64_t* __restrict__ aln_off,
                                                         const int32_t* __restrict__ ref_start, const uint64_t* __restrict__ p_ref,
                                                         const uint64_t* __restrict__ p_qry, const uint32_t* __restrict__ q_aln,
                                                         const int64_t* __restrict__ q_ref, uint32_t n_q, uint32_t* __restrict__ out_query,
                                                         uint8_t* __restrict__ out_state) {
    const uint32_t q = blockIdx.x * kThreads + threadIdx.x;
    if (q >= n_q) return;
    const uint32_t aln = q_aln[q];  // (< n_aln: the entry refuses others)
    const uint64_t b = aln_off[aln], e = aln_off[aln + 1];
    const int64_t r = q_ref[q], start = ref_start[aln];
    uint32_t query = 0;
    uint8_t state = SVX_LIFT_OUTSIDE;
    if (r >= start && e > b) {
        const uint64_t base_ref = b ? p_ref[b - 1] : 0, base_qry = b ? p_qry[b - 1] : 0;
        const uint64_t end_ref = p_ref[e - 1];
        const uint64_t target = base_ref + ((uint64_t)r - (uint64_t)start);  // (the difference < 2^63 + 2^31, base_ref < 2^60: no wrap)
        if (target < end_ref) {
            const uint64_t a = upper_bound(p_ref, b, e, target);  // the first op with P_ref > target
            const uint64_t ref_before = a > b ? p_ref[a - 1] : base_ref, qry_before = (a > b ? p_qry[a - 1] : base_qry) - base_qry;
            if ((kQryOps >> (cigar[a] & 15u)) & 1u) {
                query = (uint32_t)(qry_before + (target - ref_before));
                state = SVX_LIFT_ALIGNED;
            } else {  // D / N: the next aligned base
                query = (uint32_t)qry_before;
                state = SVX_LIFT_DELETED;
            }
        } else if (target == end_ref && end_ref > base_ref) {
            // the last op that consumes reference: the first one whose P_ref reaches the alignment's total — on integers
            // P_ref >= end_ref is P_ref > end_ref - 1, and end_ref > base_ref >= 0 here, so end_ref - 1 does not wrap
            const uint64_t a = upper_bound(p_ref, b, e, end_ref - 1);
            query = (uint32_t)(p_qry[a] - base_qry);
            state = SVX_LIFT_END;
        }
    }
    out_query[q] = query;
    out_state[q] = state;
}

// the host-side refusals of both entries
int check_lift(svx_ctx* ctx, const char* who, const uint32_t* cigar, const uint32_t* d_pool, uint64_t pool_ops, const uint64_t* aln_off,
               uint32_t n_aln, const uint32_t* q_aln, uint32_t n_q, uint64_t* n_ops) {
    SVX_TRY(svx_lift_check_offsets(ctx, who, aln_off, n_aln, cigar, d_pool, pool_ops, n_ops));
    for (uint32_t q = 0; q < n_q; ++q)
        if (q_aln[q] >= n_aln) {
            SVX_SET_ERR(ctx, "%s: query %u names alignment %u of %u", who, q, q_aln[q], n_aln);
            return SVX_E_INVALID;
        }
    return SVX_OK;
}

// cigar: host words (d_pool null) or the pool in HBM
int lift(svx_ctx* ctx, const char* who, const uint32_t* cigar, const uint32_t* d_pool, uint64_t pool_ops, const uint64_t* aln_off,
         const int32_t* ref_start, uint32_t n_aln, const uint32_t* q_aln, const int64_t* q_ref, uint32_t n_q, uint32_t* out_query,
         uint8_t* out_state) {
    if (!ctx) return SVX_E_INVALID;
    if (n_q == 0) return SVX_OK;
    if (!aln_off || !q_aln || !q_ref || !out_query || !out_state || (n_aln && !ref_start)) return SVX_E_INVALID;
    uint64_t n_ops;
    SVX_TRY(check_lift(ctx, who, cigar, d_pool, pool_ops, aln_off, n_aln, q_aln, n_q, &n_ops));
    if (n_ops == 0) {  // alignments without ops only
        memset(out_query, 0, (size_t)n_q * 4);
        memset(out_state, SVX_LIFT_OUTSIDE, n_q);
        return SVX_OK;
    }
    const uint64_t n_chunks = (n_ops + SVX_LIFT_CHUNK - 1) / SVX_LIFT_CHUNK;
    if (n_chunks > kMaxChunks) {
        SVX_SET_ERR(ctx, "%s: %llu ops, at most %llu", who, (unsigned long long)n_ops, (unsigned long long)(kMaxChunks * SVX_LIFT_CHUNK));
        return SVX_E_TOO_LARGE;
    }
    SVX_HIP(ctx, hipSetDevice(ctx->device));
    const uint32_t* d_cigar = d_pool;
    uint64_t *d_off, *d_pref, *d_pqry;
    int32_t* d_start;
    uint32_t *d_qaln, *d_query;
    int64_t* d_qref;
    uint8_t* d_state;
    Use *d_sum, *d_base;
    svx_takes st, ws;
    if (!d_pool) st.add_up(&d_cigar, cigar, n_ops);
    st.add_up(&d_off, aln_off, (size_t)n_aln + 1);
    st.add_up(&d_start, ref_start, n_aln);
    st.add_up(&d_qaln, q_aln, n_q);
    st.add_up(&d_qref, q_ref, n_q);
    st.add(&d_query, n_q);
    st.add(&d_state, n_q);
    ws.add(&d_pref, n_ops);
    ws.add(&d_pqry, n_ops);
    ws.add(&d_sum, n_chunks);
    ws.add(&d_base, n_chunks);
    SVX_TRY(svx_stage_lay(ctx, st));
    SVX_TRY(svx_ws_lay(ctx, ws));
    SVX_TRY(svx_timing_begin(ctx));
    SVX_TRY(svx_timing_mark(ctx, 1));
    SVX_TRY(svx_lift_prefixes(ctx, d_cigar, n_ops, d_sum, d_base, d_pref, d_pqry));
    SVX_TRY(svx_timing_mark(ctx, 2));
    hipLaunchKernelGGL(k_lift_query, dim3((n_q + kThreads - 1) / kThreads), dim3(kThreads), 0, ctx->stream, d_cigar, d_off, d_start, d_pref,
                       d_pqry, d_qaln, d_qref, n_q, d_query, d_state);
    SVX_HIP(ctx, hipGetLastError());
    SVX_TRY(svx_timing_end(ctx));
    SVX_TRY(svx_download(ctx, out_query, d_query, n_q));
    SVX_TRY(svx_download(ctx, out_state, d_state, n_q));
    SVX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SVX_OK;
}

}  // namespace

// ---- what svx_mismatch.hip shares with this file (svx_internal.h)
int svx_lift_check_offsets(svx_ctx* ctx, const char* who, const uint64_t* aln_off, uint32_t n_aln, const uint32_t* cigar,
                           const uint32_t* d_pool, uint64_t pool_ops, uint64_t* n_ops) {
    if (aln_off[0] != 0) {
        SVX_SET_ERR(ctx, "%s: aln_off[0] is %llu, not 0", who, (unsigned long long)aln_off[0]);
        return SVX_E_INVALID;
    }
    for (uint32_t a = 0; a < n_aln; ++a)
        if (aln_off[a + 1] < aln_off[a]) {
            SVX_SET_ERR(ctx, "%s: aln_off decreases at alignment %u", who, a);
            return SVX_E_INVALID;
        }
    *n_ops = aln_off[n_aln];
    if (d_pool ? *n_ops > pool_ops : (*n_ops && !cigar)) {
        SVX_SET_ERR(ctx, "%s: aln_off ends at %llu, behind the pool", who, (unsigned long long)*n_ops);
        return SVX_E_INVALID;
    }
    return SVX_OK;
}

int svx_lift_prefixes(svx_ctx* ctx, const uint32_t* d_cigar, uint64_t n_ops, svx_use* d_sum, svx_use* d_base, uint64_t* d_pref,
                      uint64_t* d_pqry) {
    const uint32_t n_chunks = (uint32_t)((n_ops + SVX_LIFT_CHUNK - 1) / SVX_LIFT_CHUNK);
    hipLaunchKernelGGL(k_lift_sums, dim3(n_chunks), dim3(kThreads), 0, ctx->stream, d_cigar, n_ops, d_sum);
    SVX_HIP(ctx, hipGetLastError());
    SVX_TRY(svx_lift_exclusive(ctx, d_sum, n_chunks, d_base));
    hipLaunchKernelGGL(k_lift_apply, dim3(n_chunks), dim3(kThreads), 0, ctx->stream, d_cigar, n_ops, d_base, d_pref, d_pqry);
    SVX_HIP(ctx, hipGetLastError());
    return SVX_OK;
}

int svx_lift_exclusive(svx_ctx* ctx, const svx_use* d_in, uint32_t n, svx_use* d_out) {
    hipLaunchKernelGGL(k_lift_chunks, dim3(1), dim3(kThreads), 0, ctx->stream, d_in, n, d_out);
    SVX_HIP(ctx, hipGetLastError());
    return SVX_OK;
}

extern "C" int svx_cigar_lift(svx_ctx* ctx, const uint32_t* cigar, const uint64_t* aln_off, const int32_t* ref_start, uint32_t n_aln,
                              const uint32_t* q_aln, const int64_t* q_ref, uint32_t n_q, uint32_t* out_query, uint8_t* out_state) {
    return lift(ctx, "svx_cigar_lift", cigar, nullptr, 0, aln_off, ref_start, n_aln, q_aln, q_ref, n_q, out_query, out_state);
}

extern "C" int svx_cigar_lift_dev(svx_ctx* ctx, const uint32_t* d_cigar, uint64_t n_ops, const uint64_t* aln_off, const int32_t* ref_start,
                                  uint32_t n_aln, const uint32_t* q_aln, const int64_t* q_ref, uint32_t n_q, uint32_t* out_query,
                                  uint8_t* out_state) {
    if (!d_cigar && n_ops) return SVX_E_INVALID;
    return lift(ctx, "svx_cigar_lift_dev", nullptr, d_cigar, n_ops, aln_off, ref_start, n_aln, q_aln, q_ref, n_q, out_query, out_state);
}
