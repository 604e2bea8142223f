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
//   k_cover_scan    one workgroup per list: the carried scan of svx_scan_dev.h under max over the end keys, into the
//                   context workspace;
//   k_cover_search  one lane per window, the lists in turn: upper bound of lo among the start keys (the list is read
//                   through L2, neighbouring lanes share the upper levels of the search), one compare with the prefix
//                   maximum in front of it, one byte out — consecutive lanes, consecutive bytes.
// Every word of the prefix maxima is written by the scan before the search reads it, and only inside the lists'
// ranges: nothing depends on what the workspace held (the scratch contract, include/svx.h).
//
// svx_cover_locate answers the same batch with WHICH entry covers: k_locate_scan is the carried scan under
// arg-max over (end key, list-local index) pairs — the lowest index among equal keys —, k_locate_search the same search
// that writes the index in front of the upper bound where its key reaches hi, SVX_COVER_NONE elsewhere.
//
// svx_cover_single asks of the same lists where EXACTLY one entry lies over the reference: the maximal
// ranges on which one entry, and the same one, is the only one with start <= p < end.  With the entries in start order
// slot k is [s_k, s_k+1) (the last one open to the right); only entries 0..k can be active inside it, so with
// m1 >= m2 the two largest end keys of the prefix 0..k the depth is 1 on [max(s_k, m2), min(s_k+1, m1)) and nowhere
// else in the slot: at most one segment per slot, no sort, contig borders for free as above.  Three launches:
//   k_single_scan     one workgroup per list, kChunk slots per pass: the inclusive scan of (m1, m2) under "top two of
//                     the four" on the same ladder — NOT idempotent, so every combine is over disjoint lane ranges —,
//                     one candidate segment per slot, a flag, the workgroup's exclusive sum of the flags with a running
//                     count, the segments compacted list-locally into the workspace at list_off[l] + rank; the count;
//   k_single_offsets  one workgroup: seg_off = exclusive sum of the counts over the lists, the carried scan under sum;
//   k_single_pack     every list's segments to their final contiguous place.
// A list's pack reads the `count` words its scan wrote and nothing else.
#include "svx_internal.h"
#include "svx_scan_dev.h"

namespace {

constexpr int kThreads = kScanThreads;
constexpr int kPer = kScanPer;  // consecutive elements of one thread
constexpr int kWaves = kScanWaves;
static_assert(SVX_COVER_SCAN_CHUNK == kScanChunk, "the public chunk is one pass of the carried scan");
constexpr uint32_t kMaxGridY = 65535;

// the two largest end keys of a set of entries, m1 >= m2; (0, 0): no entry
struct Top2 {
    uint64_t m1, m2;
};
// top two of the four: an element folded in twice would read as depth 2 — disjoint operands only
struct OpTop2 {
    __device__ __forceinline__ Top2 operator()(Top2 a, Top2 b) const {
        return Top2{max64(a.m1, b.m1), max64(min64(a.m1, b.m1), max64(a.m2, b.m2))};
    }
};
// the largest end key of a set of entries and the list-local index of the entry that holds it, the lowest index among
// equal keys; (0, 0): no entry — entry 0 is in every non-empty prefix, so a maximum of 0 is held by index 0 at the latest
struct ArgMax {
    uint64_t key;
    uint32_t idx, pad;
};
struct OpArgMax {
    __device__ __forceinline__ ArgMax operator()(ArgMax a, ArgMax b) const {
        return (a.key > b.key || (a.key == b.key && a.idx <= b.idx)) ? a : b;
    }
};

__global__ __launch_bounds__(kThreads) void k_cover_scan(const uint64_t* __restrict__ end_key, const uint64_t* __restrict__ list_off,
                                                         uint64_t* __restrict__ pmax) {
    __shared__ uint64_t s_wave[2][kWaves];
    carried_scan(list_off[blockIdx.x], list_off[blockIdx.x + 1], OpMax(), [=](uint64_t i) { return end_key[i]; },
                 [=](uint64_t i, uint64_t, uint64_t incl) { pmax[i] = incl; }, s_wave);
}

// one lane per query, the lists in turn: answer(i, hi) of the last entry i with start key <= lo, `none` where the list has
// no such entry
template <typename Out, typename Answer>
__device__ __forceinline__ void search_lists(const uint64_t* __restrict__ start_key, const uint64_t* __restrict__ list_off, uint32_t n_lists,
                                             const uint64_t* __restrict__ q_lo, const uint64_t* __restrict__ q_hi, uint32_t n_q,
                                             Out* __restrict__ out, Out none, Answer answer) {
    const uint32_t q = blockIdx.x * kThreads + threadIdx.x;
    if (q >= n_q) return;
    const uint64_t lo = q_lo[q], hi = q_hi[q];
    for (uint32_t l = blockIdx.y; l < n_lists; l += gridDim.y) {
        const uint64_t b = list_off[l];
        const uint64_t a = upper_bound(start_key, b, list_off[l + 1], lo);
        out[(size_t)l * n_q + q] = a > b ? answer(a - 1, hi) : none;
    }
}

__global__ __launch_bounds__(kThreads) void k_cover_search(const uint64_t* __restrict__ start_key, const uint64_t* __restrict__ pmax,
                                                           const uint64_t* __restrict__ list_off, uint32_t n_lists,
                                                           const uint64_t* __restrict__ q_lo, const uint64_t* __restrict__ q_hi,
                                                           uint32_t n_q, uint8_t* __restrict__ out) {
    search_lists(start_key, list_off, n_lists, q_lo, q_hi, n_q, out, (uint8_t)0,
                 [=](uint64_t i, uint64_t hi) { return (uint8_t)(pmax[i] >= hi ? 1 : 0); });
}

// svx_cover_locate: amax / aidx[i] is the arg-max pair of the list's entries up to i
__global__ __launch_bounds__(kThreads) void k_locate_scan(const uint64_t* __restrict__ end_key, const uint64_t* __restrict__ list_off,
                                                          uint64_t* __restrict__ amax, uint32_t* __restrict__ aidx) {
    __shared__ ArgMax s_wave[2][kWaves];
    const uint64_t lo = list_off[blockIdx.x];
    carried_scan(lo, list_off[blockIdx.x + 1], OpArgMax(), [=](uint64_t i) { return ArgMax{end_key[i], (uint32_t)(i - lo), 0}; },
                 [=](uint64_t i, ArgMax, ArgMax incl) {
                     amax[i] = incl.key;
                     aidx[i] = incl.idx;
                 },
                 s_wave);
}

__global__ __launch_bounds__(kThreads) void k_locate_search(const uint64_t* __restrict__ start_key, const uint64_t* __restrict__ amax,
                                                            const uint32_t* __restrict__ aidx, const uint64_t* __restrict__ list_off,
                                                            uint32_t n_lists, const uint64_t* __restrict__ q_lo,
                                                            const uint64_t* __restrict__ q_hi, uint32_t n_q, uint32_t* __restrict__ out) {
    search_lists(start_key, list_off, n_lists, q_lo, q_hi, n_q, out, (uint32_t)SVX_COVER_NONE,
                 [=](uint64_t i, uint64_t hi) { return amax[i] >= hi ? aidx[i] : (uint32_t)SVX_COVER_NONE; });
}

__global__ __launch_bounds__(kThreads) void k_single_scan(const uint64_t* __restrict__ start_key, const uint64_t* __restrict__ end_key,
                                                          const uint64_t* __restrict__ list_off, uint64_t* __restrict__ loc_lo,
                                                          uint64_t* __restrict__ loc_hi, uint64_t* __restrict__ count) {
    __shared__ Top2 s_top[kWaves];
    __shared__ uint64_t s_cnt[kWaves];
    const uint64_t lo = list_off[blockIdx.x], hi = list_off[blockIdx.x + 1];
    const int tid = (int)threadIdx.x;
    Top2 carry = Top2{0, 0};
    uint64_t written = 0;
    // (the trip count depends on the list alone: every lane of the group takes every pass, DPP and barriers included;
    //  s_top is written in front of the first barrier of a pass and read between the two, s_cnt written between them and
    //  read behind the second: whoever writes either again has passed the barrier behind its last read)
    for (uint64_t base = lo; base < hi; base += SVX_COVER_SCAN_CHUNK) {
        const uint64_t first = base + (uint64_t)tid * kPer;
        // slot j is [s[j], s[j + 1]): one start more than entries, UINT64_MAX behind the list's last
        uint64_t s[kPer + 1];
        Top2 t[kPer];
#pragma unroll
        for (int j = 0; j <= kPer; ++j) s[j] = first + j < hi ? start_key[first + j] : UINT64_MAX;
#pragma unroll
        for (int j = 0; j < kPer; ++j) t[j] = Top2{first + j < hi ? end_key[first + j] : 0, 0};
#pragma unroll
        for (int j = 1; j < kPer; ++j) t[j] = OpTop2()(t[j], t[j - 1]);
        Top2 total;
        Top2 before = group_before(wave_scan(t[kPer - 1], OpTop2()), s_top, tid, OpTop2(), &total);
        before = OpTop2()(before, carry);
        carry = OpTop2()(carry, total);
        uint64_t seg_lo[kPer], seg_hi[kPer];
        uint32_t mine = 0;
#pragma unroll
        for (int j = 0; j < kPer; ++j) {
            const Top2 m = OpTop2()(t[j], before);
            seg_lo[j] = max64(s[j], m.m2);
            seg_hi[j] = min64(s[j + 1], m.m1);
            if (first + j >= hi) seg_hi[j] = 0;  // (no slot: seg_lo is UINT64_MAX there)
            mine += seg_lo[j] < seg_hi[j] ? 1u : 0u;
        }
        uint64_t flagged;
        uint64_t rank = group_before(wave_scan((uint64_t)mine, OpAdd()), s_cnt, tid, OpAdd(), &flagged);
        // list-local: rank <= the slot's own index, so the stores stay inside [lo, hi)
        rank += lo + written;
#pragma unroll
        for (int j = 0; j < kPer; ++j)
            if (seg_lo[j] < seg_hi[j]) {
                loc_lo[rank] = seg_lo[j];
                loc_hi[rank] = seg_hi[j];
                ++rank;
            }
        written += flagged;
    }
    if (tid == 0) count[blockIdx.x] = written;
}

// seg_off[0] = 0, seg_off[l + 1] = count[0] + .. + count[l]: one workgroup
__global__ __launch_bounds__(kThreads) void k_single_offsets(const uint64_t* __restrict__ count, uint32_t n_lists,
                                                             uint64_t* __restrict__ seg_off) {
    __shared__ uint64_t s_wave[2][kWaves];
    if (threadIdx.x == 0) seg_off[0] = 0;
    carried_scan(0, n_lists, OpAdd(), [=](uint64_t i) { return count[i]; },
                 [=](uint64_t i, uint64_t, uint64_t incl) { seg_off[i + 1] = incl; }, s_wave);
}

__global__ __launch_bounds__(kThreads) void k_single_pack(const uint64_t* __restrict__ list_off, const uint64_t* __restrict__ seg_off,
                                                          const uint64_t* __restrict__ loc_lo, const uint64_t* __restrict__ loc_hi,
                                                          uint64_t* __restrict__ seg_lo, uint64_t* __restrict__ seg_hi) {
    const uint64_t from = list_off[blockIdx.x], to = seg_off[blockIdx.x], n = seg_off[blockIdx.x + 1] - to;
    for (uint64_t i = (uint64_t)blockIdx.y * kThreads + threadIdx.x; i < n; i += (uint64_t)gridDim.y * kThreads) {
        seg_lo[to + i] = loc_lo[from + i];
        seg_hi[to + i] = loc_hi[from + i];
    }
}

constexpr uint32_t kPackGridY = 4;
constexpr uint32_t kMaxGridX = 0x7FFFFFFFu;

// What both entries require of their lists (host pointers): offsets from 0 that never decrease, every list sorted by
// start key, every entry on one contig — and, for the entry that asks, no entry with end <= start.
int check_lists(svx_ctx* ctx, const char* who, const uint64_t* start_key, const uint64_t* end_key, const uint64_t* list_off,
                uint32_t n_lists, bool refuse_empty) {
    if (list_off[0] != 0) {
        SVX_SET_ERR(ctx, "%s: list_off[0] is %llu, not 0", who, (unsigned long long)list_off[0]);
        return SVX_E_INVALID;
    }
    for (uint32_t l = 0; l < n_lists; ++l)
        if (list_off[l + 1] < list_off[l]) {
            SVX_SET_ERR(ctx, "%s: list_off decreases at list %u", who, l);
            return SVX_E_INVALID;
        }
    if (list_off[n_lists] && (!start_key || !end_key)) return SVX_E_INVALID;
    for (uint32_t l = 0; l < n_lists; ++l)
        for (uint64_t i = list_off[l]; i < list_off[l + 1]; ++i) {
            if (i > list_off[l] && start_key[i] < start_key[i - 1]) {
                SVX_SET_ERR(ctx, "%s: list %u is not sorted by start key at entry %llu", who, l, (unsigned long long)(i - list_off[l]));
                return SVX_E_INVALID;
            }
            if ((start_key[i] >> 32) != (end_key[i] >> 32)) {
                SVX_SET_ERR(ctx, "%s: entry %llu of list %u starts and ends on different contigs", who,
                            (unsigned long long)(i - list_off[l]), l);
                return SVX_E_INVALID;
            }
            if (refuse_empty && end_key[i] <= start_key[i]) {
                SVX_SET_ERR(ctx, "%s: entry %llu of list %u ends at or in front of its start", who, (unsigned long long)(i - list_off[l]), l);
                return SVX_E_INVALID;
            }
        }
    return SVX_OK;
}

// What svx_cover_query and svx_cover_locate require of a batch (n_lists and n_q above 0): check_lists, and every query
// on one contig with lo <= hi.
int check_batch(svx_ctx* ctx, const char* who, const uint64_t* start_key, const uint64_t* end_key, const uint64_t* list_off,
                uint32_t n_lists, const uint64_t* q_lo, const uint64_t* q_hi, uint32_t n_q, const void* out) {
    if (!list_off || !q_lo || !q_hi || !out) return SVX_E_INVALID;
    SVX_TRY(check_lists(ctx, who, start_key, end_key, list_off, n_lists, false));
    for (uint32_t q = 0; q < n_q; ++q) {
        if ((q_lo[q] >> 32) != (q_hi[q] >> 32)) {
            SVX_SET_ERR(ctx, "%s: query %u starts and ends on different contigs", who, q);
            return SVX_E_INVALID;
        }
        if (q_lo[q] > q_hi[q]) {
            SVX_SET_ERR(ctx, "%s: query %u has lo > hi", who, q);
            return SVX_E_INVALID;
        }
    }
    return SVX_OK;
}

// the lists of a batch in the stage: what all three entries upload
struct DevLists {
    uint64_t *start, *end, *off;
};
void add_lists(svx_takes& st, const uint64_t* start_key, const uint64_t* end_key, const uint64_t* list_off, uint32_t n_lists, DevLists* d) {
    const uint64_t n = list_off[n_lists];
    st.add_up(&d->start, start_key, n);
    st.add_up(&d->end, end_key, n);
    st.add_up(&d->off, list_off, (size_t)n_lists + 1);
}

// svx_cover_query (one byte per answer, prefix maxima alone in the workspace) and svx_cover_locate (`locate`: four bytes
// per answer, the prefix arg-max's index array beside the maxima, lists of at most `list_limit` entries); `fill`: the byte
// of every answer where all lists are empty
int cover_batch(svx_ctx* ctx, const char* who, const uint64_t* start_key, const uint64_t* end_key, const uint64_t* list_off,
                uint32_t n_lists, const uint64_t* q_lo, const uint64_t* q_hi, uint32_t n_q, void* out, bool locate, uint64_t list_limit,
                int fill) {
    if (!ctx) return SVX_E_INVALID;
    if (n_lists == 0 || n_q == 0) return SVX_OK;
    SVX_TRY(check_batch(ctx, who, start_key, end_key, list_off, n_lists, q_lo, q_hi, n_q, out));
    const uint64_t n = list_off[n_lists];
    for (uint32_t l = 0; l < n_lists; ++l)
        if (list_off[l + 1] - list_off[l] > list_limit) {
            SVX_SET_ERR(ctx, "%s: list %u has %llu entries", who, l, (unsigned long long)(list_off[l + 1] - list_off[l]));
            return SVX_E_TOO_LARGE;
        }
    const size_t out_elem = locate ? 4 : 1, n_out = (size_t)n_lists * n_q;
    if (n == 0) {  // empty lists only
        memset(out, fill, n_out * out_elem);
        return SVX_OK;
    }
    SVX_HIP(ctx, hipSetDevice(ctx->device));
    DevLists d;
    uint64_t *d_lo, *d_hi, *d_max;
    uint8_t* d_out;
    uint32_t* d_idx = nullptr;
    svx_takes st, ws;
    add_lists(st, start_key, end_key, list_off, n_lists, &d);
    st.add_up(&d_lo, q_lo, n_q);
    st.add_up(&d_hi, q_hi, n_q);
    st.add(&d_out, n_out * out_elem);
    ws.add(&d_max, n);
    if (locate) ws.add(&d_idx, n);
    SVX_TRY(svx_stage_lay(ctx, st));
    SVX_TRY(svx_ws_lay(ctx, ws));
    SVX_TRY(svx_timing_begin(ctx));
    if (locate)
        hipLaunchKernelGGL(k_locate_scan, dim3(n_lists), dim3(kThreads), 0, ctx->stream, d.end, d.off, d_max, d_idx);
    else
        hipLaunchKernelGGL(k_cover_scan, dim3(n_lists), dim3(kThreads), 0, ctx->stream, d.end, d.off, d_max);
    SVX_HIP(ctx, hipGetLastError());
    SVX_TRY(svx_timing_mark(ctx, 1));
    const dim3 grid((n_q + kThreads - 1) / kThreads, n_lists < kMaxGridY ? n_lists : kMaxGridY);
    if (locate)
        hipLaunchKernelGGL(k_locate_search, grid, dim3(kThreads), 0, ctx->stream, d.start, d_max, d_idx, d.off, n_lists, d_lo, d_hi, n_q,
                           reinterpret_cast<uint32_t*>(d_out));
    else
        hipLaunchKernelGGL(k_cover_search, grid, dim3(kThreads), 0, ctx->stream, d.start, d_max, d.off, n_lists, d_lo, d_hi, n_q, d_out);
    SVX_HIP(ctx, hipGetLastError());
    SVX_TRY(svx_timing_mark(ctx, 2));
    SVX_TRY(svx_timing_end(ctx));
    SVX_TRY(svx_download(ctx, static_cast<uint8_t*>(out), d_out, n_out * out_elem));
    SVX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SVX_OK;
}

}  // namespace

extern "C" int svx_cover_query(svx_ctx* ctx, const uint64_t* start_key, const uint64_t* end_key, const uint64_t* list_off,
                               uint32_t n_lists, const uint64_t* q_lo, const uint64_t* q_hi, uint32_t n_q, uint8_t* out) {
    return cover_batch(ctx, "svx_cover_query", start_key, end_key, list_off, n_lists, q_lo, q_hi, n_q, out, false, UINT64_MAX, 0);
}

extern "C" int svx_cover_locate(svx_ctx* ctx, const uint64_t* start_key, const uint64_t* end_key, const uint64_t* list_off,
                                uint32_t n_lists, const uint64_t* q_lo, const uint64_t* q_hi, uint32_t n_q, uint32_t* out) {
    // (an index has to differ from "none")
    return cover_batch(ctx, "svx_cover_locate", start_key, end_key, list_off, n_lists, q_lo, q_hi, n_q, out, true, SVX_COVER_NONE - 1u, 0xFF);
}

extern "C" int svx_cover_single(svx_ctx* ctx, const uint64_t* start_key, const uint64_t* end_key, const uint64_t* list_off,
                                uint32_t n_lists, uint64_t* seg_lo, uint64_t* seg_hi, uint64_t* seg_off) {
    if (!ctx || !seg_off) return SVX_E_INVALID;
    seg_off[0] = 0;
    if (n_lists == 0) return SVX_OK;
    if (!list_off) return SVX_E_INVALID;
    SVX_TRY(check_lists(ctx, "svx_cover_single", start_key, end_key, list_off, n_lists, true));
    const uint64_t n = list_off[n_lists];
    if (n == 0) {  // empty lists only
        memset(seg_off, 0, ((size_t)n_lists + 1) * 8);
        return SVX_OK;
    }
    if (!seg_lo || !seg_hi) return SVX_E_INVALID;
    if (n_lists > kMaxGridX) {
        SVX_SET_ERR(ctx, "svx_cover_single: %u lists, at most %u", n_lists, kMaxGridX);
        return SVX_E_TOO_LARGE;
    }
    SVX_HIP(ctx, hipSetDevice(ctx->device));
    DevLists d;
    uint64_t *d_seg_lo, *d_seg_hi, *d_seg_off, *d_loc_lo, *d_loc_hi, *d_count;
    svx_takes st, ws;
    add_lists(st, start_key, end_key, list_off, n_lists, &d);
    st.add(&d_seg_lo, n);
    st.add(&d_seg_hi, n);
    st.add(&d_seg_off, (size_t)n_lists + 1);
    ws.add(&d_loc_lo, n);
    ws.add(&d_loc_hi, n);
    ws.add(&d_count, n_lists);
    SVX_TRY(svx_stage_lay(ctx, st));
    SVX_TRY(svx_ws_lay(ctx, ws));
    SVX_TRY(svx_timing_begin(ctx));
    SVX_TRY(svx_timing_mark(ctx, 1));
    hipLaunchKernelGGL(k_single_scan, dim3(n_lists), dim3(kThreads), 0, ctx->stream, d.start, d.end, d.off, d_loc_lo, d_loc_hi, d_count);
    SVX_HIP(ctx, hipGetLastError());
    SVX_TRY(svx_timing_mark(ctx, 2));
    hipLaunchKernelGGL(k_single_offsets, dim3(1), dim3(kThreads), 0, ctx->stream, d_count, n_lists, d_seg_off);
    SVX_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_single_pack, dim3(n_lists, kPackGridY), dim3(kThreads), 0, ctx->stream, d.off, d_seg_off, d_loc_lo, d_loc_hi,
                       d_seg_lo, d_seg_hi);
    SVX_HIP(ctx, hipGetLastError());
    SVX_TRY(svx_timing_end(ctx));
    // the offsets first: they say how many segments there are to fetch
    SVX_TRY(svx_download(ctx, seg_off, d_seg_off, (size_t)n_lists + 1));
    SVX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const uint64_t n_seg = seg_off[n_lists];
    if (n_seg > n) {  // (cannot happen: at most one segment per slot)
        SVX_SET_ERR(ctx, "svx_cover_single: %llu segments of %llu entries", (unsigned long long)n_seg, (unsigned long long)n);
        return SVX_E_HIP;
    }
    if (n_seg) {
        SVX_TRY(svx_download(ctx, seg_lo, d_seg_lo, n_seg));
        SVX_TRY(svx_download(ctx, seg_hi, d_seg_hi, n_seg));
        SVX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    return SVX_OK;
}
