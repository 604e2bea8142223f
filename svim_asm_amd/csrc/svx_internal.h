// svx_internal.h — context, workspace and error plumbing shared by the HIP translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>

#include "svx.h"
#include "svx_takes.h"

struct svx_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    // growable HBM workspace (bump-allocated per call, reused across calls)
    char* ws = nullptr;
    size_t ws_bytes = 0;
    size_t ws_used = 0;
    // second, independent region for host-pointer entry points (staged inputs/outputs)
    char* stage = nullptr;
    size_t stage_bytes = 0;
    size_t stage_used = 0;
    // page-locked host block of svx_collect_batch (control block up, packed results down)
    char* hpin = nullptr;
    size_t hpin_bytes = 0;
    // timing
    bool timing = false;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    bool ev_valid = false;
    // recorded right after the streaming kernel of every cigar call (svx_ctx_wait_dominant)
    hipEvent_t ev_block = nullptr;  // svx_wait_blocking
    hipEvent_t ev_dom = nullptr;
    bool ev_dom_recorded = false;
    bool want_dom = false;
    int n_cu = 256;
    uint32_t wfa_cap = 1024;  // svx_ctx_set_edit_wavefront_cap: edits the wavefront pass of the edit distance resolves
    bool barrier_pending = false;      // a kernel with a grid barrier went out since the last svx_barrier_check
    bool barrier_timed_out = false;    // the last failed svx_ctx_sync was a wait between workgroups that ran out
    bool pair_lds_set = false;         // k_pair_single's dynamic-LDS limit raised on this context's device
    uint32_t pair_launches = 0;        // launches of k_pair_single so far: which set of arrival counters is next
    bool pair_wait_free = false;       // svx_ctx_set_pair_wait_free: sort on the plan without waits inside a launch
    uint32_t pair_retries = 0;         // host-pointer calls that were re-run on that plan after a wait ran out
    uint32_t pair_single_max = 131072;  // svx_ctx_set_pair_single_launch_max: largest batch of the one-launch pair sort
    uint64_t small_batch_ops = 1ull << 23;  // svx_ctx_set_small_batch_ops: largest batch of the two-launch CIGAR path
    bool split_chain = false;               // svx_ctx_set_split_chain: the split-segment chain as three launches
    uint32_t link_group_min = 0;            // svx_ctx_set_linkage_group_min: smallest partition of the group kernel (0: default)
    uint32_t match_group_min = 0;           // svx_ctx_set_match_group_min: fewest pairs of the matching group kernel (0: default)
    int32_t shift_lane_steps = -1;          // svx_ctx_set_shift_lane_steps: steps of the lane form of svx_indel_shift (< 0: default)
    char err[512] = {0};
};

#define SVX_SET_ERR(ctx, ...)                                   \
    do {                                                        \
        if (ctx) snprintf((ctx)->err, sizeof((ctx)->err), __VA_ARGS__); \
    } while (0)

#define SVX_HIP(ctx, call)                                                              \
    do {                                                                                \
        hipError_t e__ = (call);                                                        \
        if (e__ != hipSuccess) {                                                        \
            SVX_SET_ERR(ctx, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e__),    \
                        __FILE__, __LINE__);                                            \
            return (e__ == hipErrorOutOfMemory) ? SVX_E_NOMEM : SVX_E_HIP;              \
        }                                                                               \
    } while (0)

// Evaluate an int-returning call and pass on anything but SVX_OK.
#define SVX_TRY(expr)                     \
    do {                                  \
        const int rc__ = (expr);          \
        if (rc__ != SVX_OK) return rc__;  \
    } while (0)

// Reserve `total` bytes of workspace for this call (may reallocate; synchronises the
// stream first when it has to, so earlier kernels never lose their scratch).
int svx_ws_reserve(svx_ctx* ctx, size_t total);
// Word of the workspace header where a kernel notes that a wait for other workgroups ran out; to be called
// with the stream synchronised: SVX_OK, or SVX_E_HIP after clearing the header for the calls to come.
#define SVX_WS_BARRIER_NOTE_WORD 80
int svx_barrier_check(svx_ctx* ctx);
// The arrival counters of the pair sort in the same header: the partition sweep's pair (arrivals, leavers:
// zero between calls) and the first of k_pair_single's two sets of two, which alternate launches use in turn
#define SVX_WS_SWEEP_COUNTERS_WORD 64
#define SVX_WS_SINGLE_COUNTERS_WORD 68
int svx_stage_reserve(svx_ctx* ctx, size_t total);
// workspace bytes svx_cigar_extract*_dev / svx_segments_postpass_dev reserve for a batch (svx_collect_batch_dev sums them)
size_t svx_cigar_extract_ws_need(const svx_ctx* ctx, uint64_t n_ops);
size_t svx_postpass_ws_need(const uint32_t* read_off, uint32_t n_reads);

// The split-segment chain of one submission (the a3 fields of svx_collect_dev) with the per-read scratch slice
// size of its post-passes (svx_postpass_plan); svx_cigar_extract_chain_dev sends it out with the CIGAR path.
struct svx_a3_plan {
    const uint32_t* d_seg_src;
    const int32_t* d_seg_tid;
    const int32_t* d_seg_pos;
    const uint8_t* d_seg_rev;
    const int32_t* d_seg_qend;
    uint32_t n_segs;
    const uint32_t* d_read_off;
    uint32_t n_reads;
    const int32_t* d_contig_rank;
    uint32_t n_contigs;
    svx_seg_params params;
    svx_seg* d_segs;
    int32_t* d_read_len;
    svx_raw* d_raw;
    svx_post* d_post;
    const uint64_t* d_post_off;
    uint32_t* d_post_cnt;
    uint64_t post_stride;
    const uint32_t* d_deal;    // svx_collect_dev.d_chain_deal (nullable)
    uint32_t n_deal_blocks;
};
// Validates the host copies of read_off / out_off like svx_segments_postpass_dev and returns the uniform scratch
// slice size of the post-passes (0: the reads are too uneven for one size — take the separate launches).
int svx_postpass_plan(svx_ctx* ctx, const uint32_t* read_off, uint32_t n_reads, const uint64_t* out_off, uint64_t* stride);
int svx_cigar_extract_chain_dev(svx_ctx* ctx, const uint32_t* d_cigar, uint64_t n_ops, const uint64_t* d_aln_off, uint32_t n_aln,
                                const int32_t* d_ref_start, uint32_t min_len, svx_sig_soa d_out, uint64_t cap,
                                uint64_t* d_n_out, const svx_a3_plan* a3);

// Lay out a call's scratch (svx_takes.h): reserve the list's bytes() in the region and give every slot its address; the
// stage also enqueues the list's uploads, in list order.  A lay-out starts its region from the front, as a reserve always
// did: what an earlier one placed there is given up (work already on the stream still finishes in front of the new use).
static inline int svx_ws_lay(svx_ctx* ctx, const svx_takes& t) {
    SVX_TRY(svx_ws_reserve(ctx, t.bytes()));
    ctx->ws_used = t.place(ctx->ws, ctx->ws_used);
    return SVX_OK;
}
static inline int svx_stage_lay(svx_ctx* ctx, const svx_takes& t) {
    SVX_TRY(svx_stage_reserve(ctx, t.bytes()));
    ctx->stage_used = t.place(ctx->stage, ctx->stage_used);
    for (int i = 0; i < t.n; ++i)
        if (t.up_bytes(i))
            SVX_HIP(ctx, hipMemcpyAsync(*(void**)t.s[i].at, t.s[i].src, t.up_bytes(i), hipMemcpyHostToDevice, ctx->stream));
    return SVX_OK;
}
// `count` elements up to / down from the device on the context's stream (no element: no copy)
template <typename T>
static inline int svx_upload(svx_ctx* ctx, T* d_dst, const T* src, size_t count) {
    if (count) SVX_HIP(ctx, hipMemcpyAsync(d_dst, src, count * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
    return SVX_OK;
}
template <typename T>
static inline int svx_download(svx_ctx* ctx, T* dst, const T* d_src, size_t count) {
    if (count) SVX_HIP(ctx, hipMemcpyAsync(dst, d_src, count * sizeof(T), hipMemcpyDeviceToHost, ctx->stream));
    return SVX_OK;
}

// svx_lift.hip, shared with svx_mismatch.hip: aln_off[0] == 0, non-decreasing offsets and *n_ops = aln_off[n_aln] inside the
// pool (host words `cigar`, or `pool_ops` words at d_pool when that is not null), else SVX_E_INVALID with a message naming
// the alignment or the end; the scan of an op pool's (reference, query) consumption in three launches — per-chunk sums into
// d_sum, their exclusive scan into d_base (ceil(n_ops / SVX_LIFT_CHUNK) entries each, n_ops >= 1 and at most 2^31 - 1 chunks),
// the inclusive 64-bit prefixes of both per op into d_pref / d_pqry —; and the middle launch alone: ONE workgroup's
// exclusive scan of n (reference, query) sums, d_out[k] = d_in[0] + .. + d_in[k - 1].
struct svx_use {
    uint64_t ref, qry;
};
int svx_lift_check_offsets(svx_ctx* ctx, const char* who, const uint64_t* aln_off, uint32_t n_aln, const uint32_t* cigar,
                           const uint32_t* d_pool, uint64_t pool_ops, uint64_t* n_ops);
int svx_lift_prefixes(svx_ctx* ctx, const uint32_t* d_cigar, uint64_t n_ops, svx_use* d_sum, svx_use* d_base, uint64_t* d_pref,
                      uint64_t* d_pqry);
int svx_lift_exclusive(svx_ctx* ctx, const svx_use* d_in, uint32_t n, svx_use* d_out);

// Wait for everything enqueued on the context's stream WITHOUT spinning: an event created with hipEventBlockingSync
// puts the thread to sleep until the device signals (hipStreamSynchronize burns a CPU for the whole wait: under a
// CPU quota, milliseconds of kernel time then cost the host's other threads their share).
// svx_inflate.hip, for the BAM reader's device leg (svx_bam.cpp): hipError_t as int
// (d_tok: room for the token lists of `tok_members` members, SVX_INFLATE_TOK_STRIDE slots of 8 bytes each — the members go
//  out that many at a time; d_n_tok: a word per member; both null: the one-launch kernel)
int svx_bgzf_inflate_on_stream(void* stream, const uint8_t* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len,
                               const uint32_t* d_isize, const uint32_t* d_crc, uint32_t n_members, uint8_t* d_out,
                               const uint64_t* d_out_off, uint32_t* d_status, uint32_t* d_n_tok, void* d_tok, uint32_t tok_members);
uint32_t svx_bgzf_inflate_arena_members();  // svx_bgzf_inflate_set_arena's current value
int svx_gather_ranges_on_stream(void* stream, const uint8_t* d_src, const uint64_t* d_src_off, const uint32_t* d_len,
                                const uint64_t* d_dst_off, uint32_t n, uint8_t* d_dst);
// the operators x -> x * z^(8 * 1024 * 2^j), j = 0..5, of the CRC-32 state as 32 columns each (svx_inflate.hip; the
// folds of per-lane CRC pieces in svx_inflate.hip and svx_deflate.hip)
const uint32_t (*svx_crc32_shift_columns())[32];
int svx_wait_blocking(svx_ctx* ctx);
int svx_timing_begin(svx_ctx* ctx);           // records ev[0]
int svx_timing_mark(svx_ctx* ctx, int which); // records ev[which] (1: dominant start, 2: dominant end)
int svx_timing_end(svx_ctx* ctx);             // records ev[3]
