// svx_match.hip — batched greedy one-to-one assignment on gfx950, one lane or one workgroup per partition.
//
// A truth-set comparison matches the calls of two files partition by partition: partition p holds an
// n_base[p] x n_comp[p] matrix of haplotype edit distances (0xFFFFFFFF: the pair may not match), and the answer is the
// scan of its eligible pairs sorted by (dist, i, j) that matches a pair whenever both of its members are still free.
// The linkage kernel (svx_linkage.hip) clusters and does not assign; this one assigns.
//
// Restated as rounds, which is what both kernels run: among the pairs whose row and column are both free take the
// smallest under (dist, i, j), match it, repeat until no eligible pair is left.  (The first pair of the sorted scan
// with both members free IS that minimum, and matching it frees nothing, so the rounds visit the scan's matches in
// the scan's order.)
//
//   * k_match_lanes: ONE LANE per partition.  Almost every real partition is 1 x 1 or 1 x 2 and there are tens of
//     thousands of them.  A round scans the free rows x free columns of the matrix where the call put it; the free /
//     taken state is the output itself (match_base / match_comp, pre-set to 0xFFFFFFFF), so a lane needs no scratch.
//   * k_match_group: ONE WORKGROUP per partition of at least ctx->match_group_min pairs (svx_ctx_set_match_group_min).
//     The matrix is copied into LDS up to SVX_MATCH_LDS_PAIRS pairs and read where the call staged it in the context's
//     scratch beyond.  Every row caches its minimum (dist, j) over the free columns as one 64-bit key dist << 32 | j;
//     a round is a min-reduction of dist << 32 | i over the cached rows, and then only the rows whose cached column was
//     just taken are scanned again — the nearest-neighbour idea of k_linkage_group — by sub-groups of 1 .. 64 lanes
//     (the power of two that covers n_comp), one row each.  The cache, the list of rows to rescan and the column flags
//     sit in LDS while they fit (kAuxLdsBytes) and in the context's scratch otherwise.
// Both compare the same integers under the same order: the outputs are identical.
//
// Scratch contract (include/svx.h): every word of LDS and of context scratch is written before it is read; the
// outputs are pre-set by a memset on the stream, nothing relies on what an earlier call left.
#include "svx_internal.h"

#include <vector>

namespace {

constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr unsigned long long kNoKey = ~0ull;
constexpr int kLaneThreads = 64;
constexpr uint64_t kMaxPairs = 1ull << 20;            // largest partition (SVX_E_TOO_LARGE beyond)
constexpr uint32_t kLdsPairs = SVX_MATCH_LDS_PAIRS;   // largest matrix the group kernel keeps in LDS
constexpr size_t kLdsBytes = 160 * 1024;
constexpr size_t kHeaderBytes = 128;                  // 2 x 4 reduction slots of 8 bytes, the rescan counter
constexpr size_t kAuxLdsBytes = 24 * 1024;            // per-row / per-column state up to this size stays in LDS
constexpr uint32_t kGroupMinDefault = 9;              // the smallest measured size from which the group kernel wins

__host__ __device__ constexpr size_t align16(size_t x) { return (x + 15) / 16 * 16; }
// row keys (8 bytes a row), rows to rescan (4 a row), column flags (4 a column)
__host__ __device__ constexpr size_t aux_bytes(uint32_t nb, uint32_t nc) { return align16(12 * (size_t)nb + 4 * (size_t)nc); }
static_assert(kHeaderBytes + 4 * (size_t)kLdsPairs + kAuxLdsBytes <= kLdsBytes, "matrix and state have to fit into LDS");

__host__ __device__ inline bool takes_group(uint64_t pairs, uint32_t group_min) { return pairs >= 1 && pairs >= group_min; }
__host__ __device__ inline bool aux_in_lds(uint32_t nb, uint32_t nc) { return aux_bytes(nb, nc) <= kAuxLdsBytes; }
// bytes of context scratch a partition needs: the state of a group partition too large for LDS
__host__ __device__ inline uint64_t scratch_need(uint32_t nb, uint32_t nc, uint32_t group_min) {
    return takes_group((uint64_t)nb * nc, group_min) && !aux_in_lds(nb, nc) ? aux_bytes(nb, nc) : 0;
}
__host__ __device__ inline size_t group_lds_bytes(uint32_t nb, uint32_t nc) {
    const uint64_t pairs = (uint64_t)nb * nc;
    return kHeaderBytes + (pairs <= kLdsPairs ? align16(4 * pairs) : 0) + (aux_in_lds(nb, nc) ? aux_bytes(nb, nc) : 0);
}

// launches of the group kernel by pairs: dynamic LDS and the workgroup size are per launch, so that partitions of a
// few hundred pairs do not run one to a CU because one with its 128 KiB matrix is in the batch
struct GroupClass { uint32_t hi, threads; };
constexpr GroupClass kGroupClasses[] = {{1024, 64}, {4096, 256}, {kLdsPairs, 256}, {(uint32_t)kMaxPairs, 256}};
constexpr int kNGroupClasses = sizeof(kGroupClasses) / sizeof(kGroupClasses[0]);

struct MatchArgs {
    const uint32_t* dist;         // matrices, partition after partition
    const uint32_t* n_base;       // [n_parts]
    const uint32_t* n_comp;       // [n_parts]
    const uint64_t* dist_off;     // [n_parts] first pair of partition p
    const uint64_t* base_off;     // [n_parts] first base member of partition p
    const uint64_t* comp_off;     // [n_parts] first comp member of partition p
    const uint64_t* scratch_off;  // [n_parts] byte offset into `scratch` (group partitions with their state outside LDS)
    char* scratch;
    uint32_t n_parts;
    uint32_t* match_base;         // pre-set to 0xFFFFFFFF
    uint32_t* match_comp;
    uint32_t group_min;
    uint32_t class_lo, class_hi;  // k_match_group: the pairs of this launch
};

__global__ __launch_bounds__(kLaneThreads) void k_match_lanes(MatchArgs a) {
    const uint32_t p = blockIdx.x * kLaneThreads + threadIdx.x;
    if (p >= a.n_parts) return;
    const uint32_t nb = a.n_base[p], nc = a.n_comp[p];
    if (nb == 0 || nc == 0 || takes_group((uint64_t)nb * nc, a.group_min)) return;
    const uint32_t* __restrict__ D = a.dist + a.dist_off[p];
    uint32_t* mb = a.match_base + a.base_off[p];
    uint32_t* mc = a.match_comp + a.comp_off[p];
    const uint32_t rounds = nb < nc ? nb : nc;
    for (uint32_t r = 0; r < rounds; ++r) {
        uint32_t bd = kNone, bi = 0, bj = 0;
        for (uint32_t i = 0; i < nb; ++i) {
            if (mb[i] != kNone) continue;
            const uint32_t* row = D + (size_t)i * nc;
            for (uint32_t j = 0; j < nc; ++j) {
                const uint32_t v = row[j];
                if (v < bd && mc[j] == kNone) { bd = v; bi = i; bj = j; }  // strict <, ascending (i, j): ties keep the first
            }
        }
        if (bd == kNone) break;
        mb[bi] = bj;
        mc[bj] = bi;
    }
}

// minimum over the workgroup; every lane gets it.  `slot` is one of two buffers used in turn; the barrier inside
// also orders everything the group wrote before the call.
template <int kT>
__device__ __forceinline__ unsigned long long group_min_key(unsigned long long k, unsigned long long* red, int slot) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned long long o = __shfl_xor(k, off);
        k = o < k ? o : k;
    }
    constexpr int kW = kT / 64;
    if ((threadIdx.x & 63) == 0) red[slot * 4 + (threadIdx.x >> 6)] = k;
    __syncthreads();
    k = red[slot * 4];
#pragma unroll
    for (int w = 1; w < kW; ++w) {
        const unsigned long long o = red[slot * 4 + w];
        k = o < k ? o : k;
    }
    return k;
}

// The cached minimum of the rows list[0 .. n_list) (list == nullptr: rows 0 .. n_list): sub-groups of `width` lanes, a
// power of two, take one row each; the trip count is the same for every lane of a wave, so every shuffle has all its
// partners.
template <int kT>
__device__ __forceinline__ void scan_rows(const uint32_t* D, uint32_t nc, const uint32_t* col_taken, const uint32_t* list,
                                          uint32_t n_list, uint32_t width, unsigned long long* row_key) {
    const uint32_t n_sg = kT / width, sg = threadIdx.x / width, lane = threadIdx.x & (width - 1);
    for (uint32_t r0 = 0; r0 < n_list; r0 += n_sg) {
        const uint32_t r = r0 + sg;
        const bool live = r < n_list;
        const uint32_t i = live ? (list ? list[r] : r) : 0;
        unsigned long long best = kNoKey;
        if (live) {
            const uint32_t* row = D + (size_t)i * nc;
            for (uint32_t j = lane; j < nc; j += width) {
                const uint32_t v = row[j];
                if (v != kNone && !col_taken[j]) {
                    const unsigned long long k = ((unsigned long long)v << 32) | j;
                    best = k < best ? k : best;
                }
            }
        }
        for (uint32_t off = width >> 1; off >= 1; off >>= 1) {
            const unsigned long long o = __shfl_xor(best, (int)off);
            best = o < best ? o : best;
        }
        if (live && lane == 0) row_key[i] = best;
    }
}

template <int kT>
__global__ __launch_bounds__(kT) void k_match_group(MatchArgs a) {
    extern __shared__ __attribute__((aligned(16))) char g_mem[];
    const uint32_t p = blockIdx.x;
    const uint32_t nb = a.n_base[p], nc = a.n_comp[p];
    const uint64_t pairs64 = (uint64_t)nb * nc;
    if (!takes_group(pairs64, a.group_min) || pairs64 < a.class_lo || pairs64 > a.class_hi) return;
    const uint32_t pairs = (uint32_t)pairs64;
    const uint32_t tid = threadIdx.x;
    unsigned long long* red = reinterpret_cast<unsigned long long*>(g_mem);
    uint32_t* n_work = reinterpret_cast<uint32_t*>(g_mem + 64);
    const bool mat_lds = pairs <= kLdsPairs;
    const uint32_t* gD = a.dist + a.dist_off[p];
    uint32_t* sD = reinterpret_cast<uint32_t*>(g_mem + kHeaderBytes);
    const uint32_t* D = mat_lds ? sD : gD;
    char* aux = aux_in_lds(nb, nc) ? g_mem + kHeaderBytes + (mat_lds ? align16(4 * (size_t)pairs) : 0) : a.scratch + a.scratch_off[p];
    unsigned long long* row_key = reinterpret_cast<unsigned long long*>(aux);  // dist << 32 | j of the row's best free column
    uint32_t* work = reinterpret_cast<uint32_t*>(aux + 8 * (size_t)nb);        // rows to scan again this round
    uint32_t* col_taken = work + nb;
    uint32_t* mb = a.match_base + a.base_off[p];
    uint32_t* mc = a.match_comp + a.comp_off[p];
    uint32_t width = 1;
    while (width < 64 && width < nc) width <<= 1;

    if (mat_lds)
        for (uint32_t k = tid; k < pairs; k += kT) sD[k] = gD[k];
    for (uint32_t j = tid; j < nc; j += kT) col_taken[j] = 0;
    __syncthreads();
    scan_rows<kT>(D, nc, col_taken, nullptr, nb, width, row_key);
    __syncthreads();

    int slot = 0;
    for (;;) {
        if (tid == 0) *n_work = 0;
        unsigned long long best = kNoKey;
        for (uint32_t i = tid; i < nb; i += kT) {
            const unsigned long long k = row_key[i];
            if (k != kNoKey) {
                const unsigned long long c = (k & 0xFFFFFFFF00000000ull) | i;
                best = c < best ? c : best;
            }
        }
        best = group_min_key<kT>(best, red, slot);
        slot ^= 1;
        if (best == kNoKey) break;  // the same value in every lane
        const uint32_t bi = (uint32_t)best;
        const uint32_t bj = (uint32_t)row_key[bi];
        __syncthreads();  // everyone has read row bi's key before it goes
        if (tid == 0) {
            mb[bi] = bj;
            mc[bj] = bi;
            col_taken[bj] = 1;
            row_key[bi] = kNoKey;
        }
        for (uint32_t i = tid; i < nb; i += kT) {
            if (i == bi) continue;
            const unsigned long long k = row_key[i];
            if (k != kNoKey && (uint32_t)k == bj) work[atomicAdd(n_work, 1u)] = i;
        }
        __syncthreads();
        scan_rows<kT>(D, nc, col_taken, work, *n_work, width, row_key);
        __syncthreads();
    }
}

// offsets of partition p in the distance / member / scratch arrays, from the member counts: one workgroup, each thread
// a contiguous chunk
__global__ __launch_bounds__(256) void k_match_offsets(const uint32_t* n_base, const uint32_t* n_comp, uint32_t n_parts,
                                                       uint32_t group_min, uint64_t* dist_off, uint64_t* base_off,
                                                       uint64_t* comp_off, uint64_t* scratch_off) {
    __shared__ uint64_t s_d[256], s_b[256], s_c[256], s_s[256];
    const uint32_t chunk = (n_parts + 255) / 256;
    const uint32_t lo = min(n_parts, threadIdx.x * chunk), hi = min(n_parts, lo + chunk);
    uint64_t d = 0, b = 0, c = 0, sc = 0;
    for (uint32_t p = lo; p < hi; ++p) {
        const uint32_t nb = n_base[p], nc = n_comp[p];
        d += (uint64_t)nb * nc;
        b += nb;
        c += nc;
        sc += scratch_need(nb, nc, group_min);
    }
    s_d[threadIdx.x] = d; s_b[threadIdx.x] = b; s_c[threadIdx.x] = c; s_s[threadIdx.x] = sc;
    __syncthreads();
    d = b = c = sc = 0;
    for (uint32_t t = 0; t < threadIdx.x; ++t) { d += s_d[t]; b += s_b[t]; c += s_c[t]; sc += s_s[t]; }
    for (uint32_t p = lo; p < hi; ++p) {
        const uint32_t nb = n_base[p], nc = n_comp[p];
        dist_off[p] = d; base_off[p] = b; comp_off[p] = c; scratch_off[p] = sc;
        d += (uint64_t)nb * nc;
        b += nb;
        c += nc;
        sc += scratch_need(nb, nc, group_min);
    }
}

// what the host learns from the member counts: sizes of the arrays and which launches have work
struct MatchPlan {
    uint64_t n_dist = 0, n_b = 0, n_c = 0, n_scratch = 0;
    bool lanes = false;
    size_t class_lds[kNGroupClasses] = {};  // dynamic LDS of every group launch (0: no launch)
};

void plan_add(MatchPlan& pl, uint32_t nb, uint32_t nc, uint32_t group_min) {
    const uint64_t pairs = (uint64_t)nb * nc;
    pl.n_dist += pairs;
    pl.n_b += nb;
    pl.n_c += nc;
    pl.n_scratch += scratch_need(nb, nc, group_min);
    if (!takes_group(pairs, group_min)) { pl.lanes = pl.lanes || pairs > 0; return; }
    for (int c = 0; c < kNGroupClasses; ++c)
        if (pairs <= kGroupClasses[c].hi) {
            const size_t lds = group_lds_bytes(nb, nc);
            pl.class_lds[c] = lds > pl.class_lds[c] ? lds : pl.class_lds[c];
            break;
        }
}

template <int kT>
int launch_group(svx_ctx* ctx, const MatchArgs& a, size_t lds) {
    // (always the whole of LDS, not this launch's size: the limit is kept per device, and another context's thread
    //  may set it between this call and the launch)
    SVX_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(k_match_group<kT>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBytes));
    hipLaunchKernelGGL(k_match_group<kT>, dim3(a.n_parts), dim3(kT), lds, ctx->stream, a);
    SVX_HIP(ctx, hipGetLastError());
    return SVX_OK;
}

int launch_all(svx_ctx* ctx, MatchArgs a, const MatchPlan& pl) {
    if (pl.lanes) {
        hipLaunchKernelGGL(k_match_lanes, dim3((a.n_parts + kLaneThreads - 1) / kLaneThreads), dim3(kLaneThreads), 0, ctx->stream, a);
        SVX_HIP(ctx, hipGetLastError());
    }
    uint32_t lo = 0;
    for (int c = 0; c < kNGroupClasses; ++c) {
        a.class_lo = lo;
        a.class_hi = kGroupClasses[c].hi;
        lo = kGroupClasses[c].hi + 1;
        if (!pl.class_lds[c]) continue;
        SVX_TRY(kGroupClasses[c].threads == 64 ? launch_group<64>(ctx, a, pl.class_lds[c]) : launch_group<256>(ctx, a, pl.class_lds[c]));
    }
    return SVX_OK;
}

}  // namespace

extern "C" int svx_ctx_set_match_group_min(svx_ctx* ctx, uint32_t pairs) {
    if (!ctx) return SVX_E_INVALID;
    ctx->match_group_min = pairs;  // (0: the default, resolved where the call plans its launches)
    return SVX_OK;
}

extern "C" int svx_match_greedy_batch(svx_ctx* ctx, const uint32_t* dist, const uint32_t* n_base, const uint32_t* n_comp,
                                      uint32_t n_parts, uint32_t* match_base, uint32_t* match_comp) {
    if (!ctx) return SVX_E_INVALID;
    if (n_parts == 0) return SVX_OK;
    if (!n_base || !n_comp) { SVX_SET_ERR(ctx, "svx_match_greedy_batch: null member counts"); return SVX_E_INVALID; }
    const uint32_t group_min = ctx->match_group_min ? ctx->match_group_min : kGroupMinDefault;
    MatchPlan pl;
    for (uint32_t p = 0; p < n_parts; ++p) {
        if ((uint64_t)n_base[p] * n_comp[p] > kMaxPairs) {
            SVX_SET_ERR(ctx, "svx_match_greedy_batch: partition %u has %u x %u pairs, more than 2^20", p, n_base[p], n_comp[p]);
            return SVX_E_TOO_LARGE;
        }
        plan_add(pl, n_base[p], n_comp[p], group_min);
    }
    if ((pl.n_dist && !dist) || (pl.n_b && !match_base) || (pl.n_c && !match_comp)) {
        SVX_SET_ERR(ctx, "svx_match_greedy_batch: null distances or outputs");
        return SVX_E_INVALID;
    }
    if (pl.n_dist == 0) {  // no pair anywhere: nothing to ask the device
        for (uint64_t i = 0; i < pl.n_b; ++i) match_base[i] = kNone;
        for (uint64_t j = 0; j < pl.n_c; ++j) match_comp[j] = kNone;
        return SVX_OK;
    }
    SVX_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n_scratch = pl.n_scratch ? pl.n_scratch : 1;
    uint32_t *d_dist, *d_nb, *d_nc, *d_mb, *d_mc;
    uint64_t *d_doff, *d_boff, *d_coff, *d_soff;
    char* d_scratch;
    svx_takes st;
    st.add_up(&d_dist, dist, pl.n_dist);
    st.add_up(&d_nb, n_base, n_parts);
    st.add_up(&d_nc, n_comp, n_parts);
    st.add(&d_doff, n_parts);
    st.add(&d_boff, n_parts);
    st.add(&d_coff, n_parts);
    st.add(&d_soff, n_parts);
    st.add(&d_mb, pl.n_b);
    st.add(&d_mc, pl.n_c);
    st.add(&d_scratch, n_scratch);
    SVX_TRY(svx_stage_lay(ctx, st));
    SVX_HIP(ctx, hipMemsetAsync(d_mb, 0xFF, pl.n_b * 4, ctx->stream));
    SVX_HIP(ctx, hipMemsetAsync(d_mc, 0xFF, pl.n_c * 4, ctx->stream));
    MatchArgs a;
    a.dist = d_dist; a.n_base = d_nb; a.n_comp = d_nc; a.dist_off = d_doff; a.base_off = d_boff; a.comp_off = d_coff;
    a.scratch_off = d_soff; a.scratch = d_scratch; a.n_parts = n_parts; a.match_base = d_mb; a.match_comp = d_mc;
    a.group_min = group_min; a.class_lo = a.class_hi = 0;
    SVX_TRY(svx_timing_begin(ctx));
    hipLaunchKernelGGL(k_match_offsets, dim3(1), dim3(256), 0, ctx->stream, d_nb, d_nc, n_parts, group_min, d_doff, d_boff,
                       d_coff, d_soff);
    SVX_HIP(ctx, hipGetLastError());
    SVX_TRY(svx_timing_mark(ctx, 1));
    SVX_TRY(launch_all(ctx, a, pl));
    SVX_TRY(svx_timing_mark(ctx, 2));
    SVX_TRY(svx_timing_end(ctx));
    SVX_TRY(svx_download(ctx, match_base, d_mb, pl.n_b));
    SVX_TRY(svx_download(ctx, match_comp, d_mc, pl.n_c));
    SVX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SVX_OK;
}
