// svx_cover.hip — "does one interval of this list contain this window?" for every (list, window) on gfx950.
//
// A cohort merge asks, for every record and every haplotype of every sample, whether ONE alignment of that haplotype's
// assembly spans the record's window (SVIM_MERGE.genotype_non_carriers): records x samples x 2
// questions against one interval list per haplotype.  Keys are contig << 32 | position, a list is sorted by its
// start keys.  With the contig in the high word
//     some i of the list has start[i] <= lo and end[i] >= hi
//         <=>  max(end[i] : start[i] <= lo) >= hi
// because an interval on an earlier contig ends below every key of the window's contig and one on a later contig
// starts above lo (intervals and windows never cross a contig: the entry refuses those).  The intervals with
// start <= lo are a PREFIX of the sorted list, so two launches answer the batch:
//   k_cover_scan    one workgroup per list: inclusive prefix maximum of the end keys, kChunk elements per pass
//                   (kPer consecutive ones per thread, DPP scan of the thread maxima across the wave, the waves'
//                   maxima through LDS, the running maximum carried from pass to pass), into the context workspace;
//   k_cover_search  one lane per window, the lists in turn: upper bound of lo among the start keys (the list is read
//                   through L2, neighbouring lanes share the upper levels of the search), one compare with the prefix
//                   maximum in front of it, one byte out — consecutive lanes, consecutive bytes.
// Every word of the prefix maxima is written by the scan before the search reads it, and only inside the lists'
// ranges: nothing depends on what the workspace held (the scratch contract, include/svx.h).
#include "svx_internal.h"

namespace {

constexpr int kThreads = 256;
constexpr int kPer = SVX_COVER_SCAN_CHUNK / kThreads;  // consecutive elements of one thread
constexpr int kWaves = kThreads / 64;
static_assert(kPer * kThreads == SVX_COVER_SCAN_CHUNK && kPer == 4, "four elements per thread, loaded as two 16-byte words");
constexpr uint32_t kMaxGridY = 65535;

// DPP lane movement (gfx9 family): 0 flows into lanes without a source — the identity of max over unsigned keys
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint64_t dpp0_64(uint64_t v) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)v, CTRL, ROW_MASK, 0xF, false);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(v >> 32), CTRL, ROW_MASK, 0xF, false);
    return (uint64_t)hi << 32 | lo;
}
__device__ __forceinline__ uint64_t max64(uint64_t a, uint64_t b) { return a > b ? a : b; }
// inclusive maximum over the lanes 0..l of the wave
__device__ __forceinline__ uint64_t wave_scan_max(uint64_t v) {
    v = max64(v, dpp0_64<0x111, 0xF>(v));  // row_shr:1
    v = max64(v, dpp0_64<0x112, 0xF>(v));  // row_shr:2
    v = max64(v, dpp0_64<0x114, 0xF>(v));  // row_shr:4
    v = max64(v, dpp0_64<0x118, 0xF>(v));  // row_shr:8
    v = max64(v, dpp0_64<0x142, 0xA>(v));  // row_bcast:15 into rows 1 and 3
    v = max64(v, dpp0_64<0x143, 0xC>(v));  // row_bcast:31 into rows 2 and 3
    return v;
}

__global__ __launch_bounds__(kThreads) void k_cover_scan(const uint64_t* __restrict__ end_key, const uint64_t* __restrict__ list_off,
                                                         uint64_t* __restrict__ pmax) {
    __shared__ uint64_t s_wave[2][kWaves];
    const uint64_t lo = list_off[blockIdx.x], hi = list_off[blockIdx.x + 1];
    const int tid = (int)threadIdx.x, wave = tid >> 6;
    uint64_t carry = 0;
    int slot = 0;
    // (the trip count depends on the list alone: every lane of the group takes every pass, DPP and barrier included)
    for (uint64_t base = lo; base < hi; base += SVX_COVER_SCAN_CHUNK, slot ^= 1) {
        const uint64_t first = base + (uint64_t)tid * kPer;
        uint64_t v[kPer];
#pragma unroll
        for (int j = 0; j < kPer; ++j) v[j] = first + j < hi ? end_key[first + j] : 0;
#pragma unroll
        for (int j = 1; j < kPer; ++j) v[j] = max64(v[j], v[j - 1]);
        const uint64_t incl = wave_scan_max(v[kPer - 1]);
        if ((tid & 63) == 63) s_wave[slot][wave] = incl;
        // the lanes in front of this one: wave_shr:1, lane 0 receives 0
        uint64_t before = dpp0_64<0x138, 0xF>(incl);
        __syncthreads();  // (two buffers in turn: the next write of this one is behind the next pass's barrier)
        uint64_t total = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            const uint64_t t = s_wave[slot][w];
            if (w < wave) before = max64(before, t);
            total = max64(total, t);
        }
        before = max64(before, carry);
#pragma unroll
        for (int j = 0; j < kPer; ++j)
            if (first + j < hi) pmax[first + j] = max64(v[j], before);
        carry = max64(carry, total);
    }
}

__global__ __launch_bounds__(kThreads) void k_cover_search(const uint64_t* __restrict__ start_key, const uint64_t* __restrict__ pmax,
                                                           const uint64_t* __restrict__ list_off, uint32_t n_lists,
                                                           const uint64_t* __restrict__ q_lo, const uint64_t* __restrict__ q_hi,
                                                           uint32_t n_q, uint8_t* __restrict__ out) {
    const uint32_t q = blockIdx.x * kThreads + threadIdx.x;
    if (q >= n_q) return;
    const uint64_t lo = q_lo[q], hi = q_hi[q];
    for (uint32_t l = blockIdx.y; l < n_lists; l += gridDim.y) {
        const uint64_t b = list_off[l], e = list_off[l + 1];
        // first element with start_key > lo
        uint64_t a = b, n = e - b;
        while (n) {
            const uint64_t half = n >> 1;
            if (start_key[a + half] <= lo) { a += half + 1; n -= half + 1; } else n = half;
        }
        out[(size_t)l * n_q + q] = (a > b && pmax[a - 1] >= hi) ? 1 : 0;
    }
}

}  // namespace

extern "C" int svx_cover_query(svx_ctx* ctx, const uint64_t* start_key, const uint64_t* end_key, const uint64_t* list_off,
                               uint32_t n_lists, const uint64_t* q_lo, const uint64_t* q_hi, uint32_t n_q, uint8_t* out) {
    if (!ctx) return SVX_E_INVALID;
    if (n_lists == 0 || n_q == 0) return SVX_OK;
    if (!list_off || !q_lo || !q_hi || !out) return SVX_E_INVALID;
    if (list_off[0] != 0) {
        SVX_SET_ERR(ctx, "svx_cover_query: list_off[0] is %llu, not 0", (unsigned long long)list_off[0]);
        return SVX_E_INVALID;
    }
    for (uint32_t l = 0; l < n_lists; ++l)
        if (list_off[l + 1] < list_off[l]) {
            SVX_SET_ERR(ctx, "svx_cover_query: list_off decreases at list %u", l);
            return SVX_E_INVALID;
        }
    const uint64_t n = list_off[n_lists];
    if (n && (!start_key || !end_key)) return SVX_E_INVALID;
    for (uint32_t l = 0; l < n_lists; ++l)
        for (uint64_t i = list_off[l]; i < list_off[l + 1]; ++i) {
            if (i > list_off[l] && start_key[i] < start_key[i - 1]) {
                SVX_SET_ERR(ctx, "svx_cover_query: list %u is not sorted by start key at entry %llu", l,
                            (unsigned long long)(i - list_off[l]));
                return SVX_E_INVALID;
            }
            if ((start_key[i] >> 32) != (end_key[i] >> 32)) {
                SVX_SET_ERR(ctx, "svx_cover_query: entry %llu of list %u starts and ends on different contigs",
                            (unsigned long long)(i - list_off[l]), l);
                return SVX_E_INVALID;
            }
        }
    for (uint32_t q = 0; q < n_q; ++q) {
        if ((q_lo[q] >> 32) != (q_hi[q] >> 32)) {
            SVX_SET_ERR(ctx, "svx_cover_query: query %u starts and ends on different contigs", q);
            return SVX_E_INVALID;
        }
        if (q_lo[q] > q_hi[q]) {
            SVX_SET_ERR(ctx, "svx_cover_query: query %u has lo > hi", q);
            return SVX_E_INVALID;
        }
    }
    const size_t n_out = (size_t)n_lists * n_q;
    if (n == 0) {  // empty lists only
        memset(out, 0, n_out);
        return SVX_OK;
    }
    SVX_HIP(ctx, hipSetDevice(ctx->device));
    int rc = svx_stage_reserve(ctx, 2 * svx_take_bytes(n, 8) + svx_take_bytes((size_t)n_lists + 1, 8) + 2 * svx_take_bytes(n_q, 8) +
                                        svx_take_bytes(n_out, 1));
    if (rc != SVX_OK) return rc;
    rc = svx_ws_reserve(ctx, svx_take_bytes(n, 8));
    if (rc != SVX_OK) return rc;
    uint64_t* d_start = svx_stage_take<uint64_t>(ctx, n);
    uint64_t* d_end = svx_stage_take<uint64_t>(ctx, n);
    uint64_t* d_off = svx_stage_take<uint64_t>(ctx, (size_t)n_lists + 1);
    uint64_t* d_lo = svx_stage_take<uint64_t>(ctx, n_q);
    uint64_t* d_hi = svx_stage_take<uint64_t>(ctx, n_q);
    uint8_t* d_out = svx_stage_take<uint8_t>(ctx, n_out);
    uint64_t* d_pmax = svx_ws_take<uint64_t>(ctx, n);
    SVX_HIP(ctx, hipMemcpyAsync(d_start, start_key, n * 8, hipMemcpyHostToDevice, ctx->stream));
    SVX_HIP(ctx, hipMemcpyAsync(d_end, end_key, n * 8, hipMemcpyHostToDevice, ctx->stream));
    SVX_HIP(ctx, hipMemcpyAsync(d_off, list_off, ((size_t)n_lists + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    SVX_HIP(ctx, hipMemcpyAsync(d_lo, q_lo, (size_t)n_q * 8, hipMemcpyHostToDevice, ctx->stream));
    SVX_HIP(ctx, hipMemcpyAsync(d_hi, q_hi, (size_t)n_q * 8, hipMemcpyHostToDevice, ctx->stream));
    rc = svx_timing_begin(ctx);
    if (rc != SVX_OK) return rc;
    hipLaunchKernelGGL(k_cover_scan, dim3(n_lists), dim3(kThreads), 0, ctx->stream, d_end, d_off, d_pmax);
    SVX_HIP(ctx, hipGetLastError());
    rc = svx_timing_mark(ctx, 1);
    if (rc != SVX_OK) return rc;
    const dim3 grid((n_q + kThreads - 1) / kThreads, n_lists < kMaxGridY ? n_lists : kMaxGridY);
    hipLaunchKernelGGL(k_cover_search, grid, dim3(kThreads), 0, ctx->stream, d_start, d_pmax, d_off, n_lists, d_lo, d_hi, n_q, d_out);
    SVX_HIP(ctx, hipGetLastError());
    rc = svx_timing_mark(ctx, 2);
    if (rc != SVX_OK) return rc;
    rc = svx_timing_end(ctx);
    if (rc != SVX_OK) return rc;
    SVX_HIP(ctx, hipMemcpyAsync(out, d_out, n_out, hipMemcpyDeviceToHost, ctx->stream));
    SVX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SVX_OK;
}
