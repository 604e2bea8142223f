// svx_linkage.hip — batched complete linkage + flat cut on gfx950, one lane or one workgroup per partition.
//
// Replaces, for every partition of the PAIR step and every group of overlapping inversion
// breakpoints of a read,
//     fcluster(linkage(distances, method="complete"), t, criterion="distance")
// (reference SVIM_COMBINE.py:134-135,155-156 and SVIM_inter.py:47-48; scipy.cluster.hierarchy).
// The flat-cluster LABELS decide which member is cluster[0], i.e. whose coordinates the paired call
// carries (SVIM_COMBINE.py:184-363), so scipy's procedure is reproduced step by step:
//   nearest-neighbour chain with its tie rules (strict <, lowest index, previous chain element
//   preferred), merged cluster keeps the larger index, complete-linkage update max(d(x,i), d(y,i));
//   stable sort of the merges by distance; union-find relabelling (smaller root first); maximum
//   distance per subtree; explicit-stack traversal from the root, left child first, numbering flat
//   clusters as the traversal completes them.
// Partitions are tiny (2..10 members in PAIR) and there are thousands of them: the work is a short
// sequential program per partition, so the mapping is one lane per partition with its whole state
// (distance matrix, merge list, union-find, stack) in a private LDS slice — no global traffic besides
// the input vector and the labels.  Partitions with more members than the LDS slice holds (inversion
// groups of pathological reads) run the same code on a slice of the HBM workspace.
// Double precision throughout (scipy computes in float64; the cut compares with <=): only
// comparisons, max and copies — no arithmetic that could round differently.
//
// A cohort merge (SVIM_MERGE.py) has partitions of dozens to hundreds of distinct alleles, thousands of them.  The
// chain is O(n²) long per lane there and every step an uncoalesced 8-byte read, so partitions of at least
// ctx->link_group_min members (svx_ctx_set_linkage_group_min) go to k_linkage_group instead: ONE WORKGROUP per
// partition, the same procedure with its data-parallel steps spread over the group —
//   * the working matrix is the FULL n x n matrix (odd row pitch), in LDS up to SVX_LINKAGE_GROUP_LDS_N members and in
//     the workspace beyond: the row of the chain top is read contiguously, one element per lane;
//   * the nearest neighbour of the chain top x is a lexicographic (distance, index) min-reduction over the live
//     i != x, taken only if its distance is strictly below D[x, y_prev] — the serial scan starts at D[x, y_prev] and
//     replaces on strict < in ascending index, so both pick the same element;
//   * the Lance–Williams update max(D[i,x], D[i,y]) goes into row y and column y, one live i per lane;
//   * the stable sort of the n - 1 merges is a rank by (distance, original index), one merge per lane;
//   * union-find relabelling, maximum below and the stack traversal stay serial: lane 0, on arrays in LDS.
// Same compares, max and copies on the same doubles: the labels are those of svx_linkage_cut_one bit for bit.
#include "svx_internal.h"
#include "svx_linkage_dev.h"

#include <vector>

namespace {

constexpr int kThreads = 64;
constexpr uint32_t kLdsN = 10;  // partitions up to this size keep their state in LDS

constexpr size_t kSlice = (svx_link_bytes(kLdsN) + 15) / 16 * 16;

// ---- the workgroup-cooperative kernel's geometry
constexpr uint32_t kGroupLdsN = SVX_LINKAGE_GROUP_LDS_N;  // largest partition whose matrix lives in LDS
constexpr uint32_t kGroupMaxN = 2048;   // largest partition of the group kernel (its per-member arrays fill LDS beyond)
constexpr uint32_t kGroupMinDefault = 16;  // the smallest measured size from which the group kernel wins
constexpr size_t kLdsBytes = 160 * 1024;

__host__ __device__ constexpr uint32_t group_pitch(uint32_t n) { return n | 1u; }  // odd: column stores spread over the banks
// per-member arrays of the group kernel: doubles zd, md, szd | ints zx, zy, sx, sy, size, chain, stack, parent[2n] |
// bytes visited[2n], plus the two reduction buffers
__host__ __device__ constexpr size_t group_aux_bytes(uint32_t n) {
    return 24 * (size_t)n + 4 * 9 * (size_t)n + ((2 * (size_t)n + 7) / 8) * 8 + 2 * 4 * 8 + 2 * 4 * 4;
}
__host__ __device__ constexpr size_t group_matrix_bytes(uint32_t n) { return 8 * (size_t)n * group_pitch(n); }
static_assert(group_matrix_bytes(kGroupLdsN) + group_aux_bytes(kGroupLdsN) <= kLdsBytes, "the LDS matrix has to fit");
static_assert(group_aux_bytes(kGroupMaxN) <= kLdsBytes, "the per-member arrays have to fit");

__host__ __device__ inline bool takes_group(uint32_t n, uint32_t group_min) { return n >= 2 && n >= group_min && n <= kGroupMaxN; }
// bytes of HBM scratch partition of n members needs (16-byte granules)
__host__ __device__ inline uint64_t scratch_need(uint32_t n, uint32_t group_min) {
    if (takes_group(n, group_min)) return n > kGroupLdsN ? (group_matrix_bytes(n) + 15) / 16 * 16 : 0;
    return n > kLdsN ? (svx_link_bytes(n) + 15) / 16 * 16 : 0;
}
// launches of the group kernel: [lo, hi] members, lanes, matrix in LDS — dynamic LDS and the workgroup size are
// per launch, so that sixty-member partitions do not run one to a CU because a thousand-member one is in the batch
struct GroupClass { uint32_t hi, threads; };
constexpr GroupClass kGroupClasses[] = {{32, 64}, {64, 64}, {kGroupLdsN, 256}, {512, 256}, {kGroupMaxN, 256}};
constexpr int kNGroupClasses = sizeof(kGroupClasses) / sizeof(kGroupClasses[0]);

struct LinkArgs {
    const double* dist;          // condensed vectors, partition after partition
    const uint64_t* dist_off;    // [n_parts] first element of partition p
    const uint32_t* n_members;   // [n_parts]
    const uint64_t* label_off;   // [n_parts] first label of partition p
    const uint64_t* scratch_off; // [n_parts] byte offset into `scratch` (large partitions only)
    char* scratch;
    uint32_t n_parts;
    double cutoff;
    uint32_t* labels;
    uint32_t group_min;          // partitions with takes_group(n, group_min) are k_linkage_group's
    uint32_t class_lo, class_hi; // k_linkage_group: the sizes of this launch
};

__global__ __launch_bounds__(kThreads) void k_linkage_cut(LinkArgs a) {
    __shared__ __attribute__((aligned(16))) char s_mem[kThreads * kSlice];
    const uint32_t p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= a.n_parts) return;
    const uint32_t n = a.n_members[p];
    if (takes_group(n, a.group_min)) return;
    char* mem = n <= kLdsN ? s_mem + (size_t)threadIdx.x * kSlice : a.scratch + a.scratch_off[p];
    svx_linkage_cut_one(n, a.dist + a.dist_off[p], a.cutoff, a.labels + a.label_off[p], mem);
}


// lexicographic (distance, index) minimum over the workgroup; every lane gets it.  `slot` is one of two buffers used
// in turn, so that one barrier per call is enough.
template <int kT>
__device__ __forceinline__ void group_min_reduce(double& d, int& i, double* red_d, int* red_i, int slot) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double od = __shfl_xor(d, off);
        const int oi = __shfl_xor(i, off);
        if (od < d || (od == d && oi < i)) { d = od; i = oi; }
    }
    if (kT > 64) {
        constexpr int kW = kT / 64;
        if ((threadIdx.x & 63) == 0) { red_d[slot * 4 + (threadIdx.x >> 6)] = d; red_i[slot * 4 + (threadIdx.x >> 6)] = i; }
        __syncthreads();
        d = red_d[slot * 4]; i = red_i[slot * 4];
#pragma unroll
        for (int w = 1; w < kW; ++w) {
            const double od = red_d[slot * 4 + w];
            const int oi = red_i[slot * 4 + w];
            if (od < d || (od == d && oi < i)) { d = od; i = oi; }
        }
    }
}

template <int kT>
__global__ __launch_bounds__(kT) void k_linkage_group(LinkArgs a) {
    extern __shared__ __attribute__((aligned(16))) char g_mem[];
    const uint32_t p = blockIdx.x;
    const uint32_t n = a.n_members[p];
    if (!takes_group(n, a.group_min) || n < a.class_lo || n > a.class_hi) return;
    const int tid = (int)threadIdx.x;
    const uint32_t ld = group_pitch(n);
    const bool in_lds = n <= kGroupLdsN;
    double* D = in_lds ? reinterpret_cast<double*>(g_mem) : reinterpret_cast<double*>(a.scratch + a.scratch_off[p]);
    double* zd = reinterpret_cast<double*>(g_mem + (in_lds ? group_matrix_bytes(n) : 0));
    double* md = zd + n;
    double* szd = md + n;
    double* red_d = szd + n;
    int* zx = reinterpret_cast<int*>(red_d + 8);
    int* zy = zx + n;
    int* sx = zy + n;
    int* sy = sx + n;
    int* size = sy + n;
    int* chain = size + n;
    int* stack = chain + n;
    int* parent = stack + n;
    int* red_i = parent + 2 * n;
    unsigned char* visited = reinterpret_cast<unsigned char*>(red_i + 8);
    const double* __restrict__ cond = a.dist + a.dist_off[p];
    const double inf = __builtin_huge_val();

    // ---- the condensed vector → both halves of the full matrix
    {
        const double* row = cond;
        for (uint32_t i = 0; i < n; ++i) {
            for (uint32_t j = i + 1 + tid; j < n; j += kT) {
                const double v = row[j - i - 1];
                D[(size_t)i * ld + j] = v;
                D[(size_t)j * ld + i] = v;
            }
            row += n - 1 - i;
        }
        for (uint32_t i = tid; i < n; i += kT) size[i] = 1;
    }
    __syncthreads();

    // ---- nearest-neighbour chain: every lane keeps the same chain_len / x / y_prev in registers
    int chain_len = 0, first_live = 0, slot = 0;
    for (uint32_t k = 0; k + 1 < n; ++k) {
        int x, y = 0, y_prev;
        double cur;
        if (chain_len == 0) {
            while (size[first_live] == 0) ++first_live;  // dead members stay dead: O(n) over the whole run
            if (tid == 0) chain[0] = first_live;
            chain_len = 1;
            x = first_live; y_prev = -1;
        } else {  // (written at least one barrier ago: the two elements above them were pushed since)
            x = chain[chain_len - 1];
            y_prev = chain_len > 1 ? chain[chain_len - 2] : -1;
        }
        for (;;) {
            const double* rx = D + (size_t)x * ld;
            if (y_prev >= 0) { y = y_prev; cur = rx[y_prev]; } else cur = inf;
            double bd = inf;
            int bi = 0x7fffffff;
            for (int i = tid; i < (int)n; i += kT) {
                if (size[i] == 0 || i == x) continue;
                const double d = rx[i];
                if (d < bd) { bd = d; bi = i; }
            }
            group_min_reduce<kT>(bd, bi, red_d, red_i, slot);
            slot ^= 1;
            if (bd < cur) { cur = bd; y = bi; }
            if (y_prev >= 0 && y == y_prev) break;
            if (tid == 0) chain[chain_len] = y;
            ++chain_len;
            y_prev = x;
            x = y;
        }
        chain_len -= 2;
        if (x > y) { const int t = x; x = y; y = t; }
        // ---- merge x into y; Lance–Williams: D[i, y] = max(D[i, x], D[i, y]) over the live i
        {
            const double* rx = D + (size_t)x * ld;
            double* ry = D + (size_t)y * ld;
            for (int i = tid; i < (int)n; i += kT) {
                if (size[i] == 0 || i == x || i == y) continue;
                const double u = rx[i], v = ry[i];
                const double m = u > v ? u : v;
                ry[i] = m;
                D[(size_t)i * ld + y] = m;
            }
        }
        if (tid == 0) {
            zx[k] = x; zy[k] = y; zd[k] = cur;
            size[y] = size[x] + size[y];
            size[x] = 0;
        }
        __syncthreads();
    }

    // ---- stable sort of the merges by distance: rank by (zd, original index)
    const int m = (int)n - 1;
    for (int i = tid; i < m; i += kT) {
        const double di = zd[i];
        int rank = 0;
        for (int j = 0; j < m; ++j) {
            const double dj = zd[j];
            rank += (dj < di || (dj == di && j < i)) ? 1 : 0;
        }
        szd[rank] = di; sx[rank] = zx[i]; sy[rank] = zy[i];
    }
    for (uint32_t i = tid; i < 2 * n - 1; i += kT) { parent[i] = (int)i; visited[i] = 0; }
    __syncthreads();

    // ---- serial: union-find relabelling, maximum below, stack traversal (labels into `chain`)
    if (tid == 0) {
        int next = (int)n;
        for (int i = 0; i < m; ++i) {
            int r0 = sx[i], r1 = sy[i];
            {
                int q = r0, root = r0;
                while (parent[root] != root) root = parent[root];
                while (parent[q] != root) { const int t = parent[q]; parent[q] = root; q = t; }
                r0 = root;
            }
            {
                int q = r1, root = r1;
                while (parent[root] != root) root = parent[root];
                while (parent[q] != root) { const int t = parent[q]; parent[q] = root; q = t; }
                r1 = root;
            }
            sx[i] = r0 < r1 ? r0 : r1;
            sy[i] = r0 < r1 ? r1 : r0;
            parent[r0] = next;
            parent[r1] = next;
            ++next;
        }
        for (int i = 0; i < m; ++i) {
            double v = szd[i];
            if (sx[i] >= (int)n && md[sx[i] - (int)n] > v) v = md[sx[i] - (int)n];
            if (sy[i] >= (int)n && md[sy[i] - (int)n] > v) v = md[sy[i] - (int)n];
            md[i] = v;
        }
        int kk = 0, n_cluster = 0, leader = -1;
        stack[0] = 2 * (int)n - 2;
        while (kk >= 0) {
            const int root = stack[kk] - (int)n;
            const int lc = sx[root], rc = sy[root];
            if (leader == -1 && md[root] <= a.cutoff) { leader = root; ++n_cluster; }
            if (lc >= (int)n && !visited[lc]) { visited[lc] = 1; stack[++kk] = lc; continue; }
            if (rc >= (int)n && !visited[rc]) { visited[rc] = 1; stack[++kk] = rc; continue; }
            if (lc < (int)n) { if (leader == -1) ++n_cluster; chain[lc] = n_cluster; }
            if (rc < (int)n) { if (leader == -1) ++n_cluster; chain[rc] = n_cluster; }
            if (leader == root) leader = -1;
            --kk;
        }
    }
    __syncthreads();
    uint32_t* labels = a.labels + a.label_off[p];
    for (uint32_t i = tid; i < n; i += kT) labels[i] = (uint32_t)chain[i];
}

// offsets of partition p in the distance / label / scratch arrays, from the member counts: one workgroup, each
// thread a contiguous chunk (the asynchronous entry point reads no host memory after it returns)
__global__ __launch_bounds__(256) void k_linkage_offsets(const uint32_t* n_members, uint32_t n_parts, uint32_t group_min,
                                                         uint64_t* dist_off, uint64_t* label_off, uint64_t* scratch_off) {
    __shared__ uint64_t s_d[256], s_l[256], s_s[256];
    const uint32_t chunk = (n_parts + 255) / 256;
    const uint32_t lo = threadIdx.x * chunk, hi = min(n_parts, lo + chunk);
    uint64_t d = 0, l = 0, sc = 0;
    for (uint32_t p = lo; p < hi; ++p) {
        const uint64_t n = n_members[p];
        d += n * (n ? n - 1 : 0) / 2;
        l += n;
        sc += scratch_need((uint32_t)n, group_min);
    }
    s_d[threadIdx.x] = d; s_l[threadIdx.x] = l; s_s[threadIdx.x] = sc;
    __syncthreads();
    d = l = sc = 0;
    for (uint32_t t = 0; t < threadIdx.x; ++t) { d += s_d[t]; l += s_l[t]; sc += s_s[t]; }
    for (uint32_t p = lo; p < hi; ++p) {
        const uint64_t n = n_members[p];
        dist_off[p] = d; label_off[p] = l; scratch_off[p] = sc;
        d += n * (n ? n - 1 : 0) / 2;
        l += n;
        sc += scratch_need((uint32_t)n, group_min);
    }
}

// what the host learns from its copy of the member counts: sizes of the arrays and which launches have work
struct LinkPlan {
    uint64_t n_dist = 0, n_lab = 0, n_scratch = 0;
    bool lanes = false;
    uint32_t class_max[kNGroupClasses] = {};  // largest partition of every group launch (0: no launch)
};

void plan_add(LinkPlan& pl, uint32_t n32, uint32_t group_min) {
    const uint64_t n = n32;
    pl.n_dist += n * (n ? n - 1 : 0) / 2;
    pl.n_lab += n;
    pl.n_scratch += scratch_need(n32, group_min);
    if (!takes_group(n32, group_min)) { pl.lanes = pl.lanes || n32 > 0; return; }
    for (int c = 0; c < kNGroupClasses; ++c)
        if (n32 <= kGroupClasses[c].hi) { pl.class_max[c] = n32 > pl.class_max[c] ? n32 : pl.class_max[c]; break; }
}

template <int kT>
int launch_group(svx_ctx* ctx, const LinkArgs& a, uint32_t n_max) {
    const size_t lds = group_aux_bytes(n_max) + (n_max <= kGroupLdsN ? group_matrix_bytes(n_max) : 0);
    // (always the whole of LDS, not this launch's size: the limit is kept per device, and another context's thread
    //  may set it between this call and the launch)
    SVX_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(k_linkage_group<kT>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBytes));
    hipLaunchKernelGGL(k_linkage_group<kT>, dim3(a.n_parts), dim3(kT), lds, ctx->stream, a);
    SVX_HIP(ctx, hipGetLastError());
    return SVX_OK;
}

// the lane kernel for the partitions that stay with it, one group launch per size class with work
int launch_all(svx_ctx* ctx, LinkArgs a, const LinkPlan& pl) {
    if (pl.lanes) {
        hipLaunchKernelGGL(k_linkage_cut, dim3((a.n_parts + kThreads - 1) / kThreads), dim3(kThreads), 0, ctx->stream, a);
        SVX_HIP(ctx, hipGetLastError());
    }
    uint32_t lo = 0;
    for (int c = 0; c < kNGroupClasses; ++c) {
        a.class_lo = lo;
        a.class_hi = kGroupClasses[c].hi;
        lo = kGroupClasses[c].hi + 1;
        if (!pl.class_max[c]) continue;
        SVX_TRY(kGroupClasses[c].threads == 64 ? launch_group<64>(ctx, a, pl.class_max[c]) : launch_group<256>(ctx, a, pl.class_max[c]));
    }
    return SVX_OK;
}

// both entries behind their offsets: the timed launches over arrays in HBM (after svx_timing_begin)
int cut_timed(svx_ctx* ctx, const double* d_dist, const uint32_t* d_n_members, const uint64_t* d_doff, const uint64_t* d_loff,
              const uint64_t* d_soff, char* d_scratch, uint32_t n_parts, double cutoff, uint32_t* d_labels, uint32_t group_min,
              const LinkPlan& pl) {
    LinkArgs a;
    a.dist = d_dist; a.dist_off = d_doff; a.n_members = d_n_members; a.label_off = d_loff; a.scratch_off = d_soff;
    a.scratch = d_scratch; a.n_parts = n_parts; a.cutoff = cutoff; a.labels = d_labels;
    a.group_min = group_min; a.class_lo = a.class_hi = 0;
    SVX_TRY(svx_timing_mark(ctx, 1));
    SVX_TRY(launch_all(ctx, a, pl));
    SVX_TRY(svx_timing_mark(ctx, 2));
    return svx_timing_end(ctx);
}

}  // namespace

extern "C" int svx_ctx_set_linkage_group_min(svx_ctx* ctx, uint32_t n) {
    if (!ctx) return SVX_E_INVALID;
    ctx->link_group_min = n == 0 ? kGroupMinDefault : n;
    return SVX_OK;
}

extern "C" int svx_linkage_cut_batch_dev(svx_ctx* ctx, const double* d_dist, const uint32_t* n_members,
                                         const uint32_t* d_n_members, uint32_t n_parts, double cutoff, uint32_t* d_labels) {
    if (!ctx) return SVX_E_INVALID;
    if (n_parts == 0) return SVX_OK;
    if (!n_members || !d_n_members || !d_labels) return SVX_E_INVALID;
    const uint32_t group_min = ctx->link_group_min ? ctx->link_group_min : kGroupMinDefault;
    LinkPlan pl;
    for (uint32_t p = 0; p < n_parts; ++p) plan_add(pl, n_members[p], group_min);
    const uint64_t n_dist = pl.n_dist, n_lab = pl.n_lab, n_scratch = pl.n_scratch;
    if (n_dist && !d_dist) return SVX_E_INVALID;
    if (n_lab == 0) return SVX_OK;
    SVX_HIP(ctx, hipSetDevice(ctx->device));
    uint64_t *d_doff, *d_loff, *d_soff;
    char* d_scratch;
    svx_takes ws;
    ws.add(&d_doff, n_parts);
    ws.add(&d_loff, n_parts);
    ws.add(&d_soff, n_parts);
    ws.add(&d_scratch, n_scratch ? n_scratch : 1);
    SVX_TRY(svx_ws_lay(ctx, ws));
    SVX_TRY(svx_timing_begin(ctx));
    hipLaunchKernelGGL(k_linkage_offsets, dim3(1), dim3(256), 0, ctx->stream, d_n_members, n_parts, group_min, d_doff, d_loff, d_soff);
    return cut_timed(ctx, d_dist, d_n_members, d_doff, d_loff, d_soff, d_scratch, n_parts, cutoff, d_labels, group_min, pl);
}

extern "C" int svx_linkage_cut_batch(svx_ctx* ctx, const double* dist, const uint32_t* n_members, uint32_t n_parts,
                                     double cutoff, uint32_t* labels) {
    if (!ctx) return SVX_E_INVALID;
    if (n_parts == 0) return SVX_OK;
    if (!n_members || !labels) return SVX_E_INVALID;
    std::vector<uint64_t> dist_off(n_parts), label_off(n_parts), scratch_off(n_parts);
    const uint32_t group_min = ctx->link_group_min ? ctx->link_group_min : kGroupMinDefault;
    LinkPlan pl;
    for (uint32_t p = 0; p < n_parts; ++p) {
        dist_off[p] = pl.n_dist;
        label_off[p] = pl.n_lab;
        scratch_off[p] = pl.n_scratch;
        plan_add(pl, n_members[p], group_min);
    }
    const uint64_t n_dist = pl.n_dist, n_lab = pl.n_lab, n_scratch = pl.n_scratch;
    if (n_dist && !dist) return SVX_E_INVALID;
    if (n_lab == 0) return SVX_OK;
    SVX_HIP(ctx, hipSetDevice(ctx->device));
    double* d_dist;
    uint64_t *d_doff, *d_loff, *d_soff;
    uint32_t *d_nm, *d_lab;
    char* d_scratch;
    svx_takes st;
    if (n_dist) st.add_up(&d_dist, dist, n_dist); else st.add(&d_dist, 1);
    st.add_up(&d_doff, dist_off.data(), n_parts);
    st.add_up(&d_loff, label_off.data(), n_parts);
    st.add_up(&d_soff, scratch_off.data(), n_parts);
    st.add_up(&d_nm, n_members, n_parts);
    st.add(&d_lab, n_lab);
    st.add(&d_scratch, n_scratch ? n_scratch : 1);
    SVX_TRY(svx_stage_lay(ctx, st));
    SVX_TRY(svx_timing_begin(ctx));
    SVX_TRY(cut_timed(ctx, d_dist, d_nm, d_doff, d_loff, d_soff, d_scratch, n_parts, cutoff, d_lab, group_min, pl));
    SVX_TRY(svx_download(ctx, labels, d_lab, n_lab));
    SVX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SVX_OK;
}
