// svx_mismatch.hip — "where does the aligned contig differ from the reference, base for base?" for a batch of alignments
// on gfx950 (svx_cigar_mismatch, include/svx.h).
//
// The definition is the loop in include/svx.h: walk an alignment's ops with lift's two cursors and compare, inside every
// M / = / X op, the reference window's byte with the SEQ byte of each column that lies inside both lengths.
//
// The unit of work is a TILE of SVX_MISMATCH_TILE consecutive reference positions of one alignment's window, one workgroup
// per tile and kCols consecutive positions per lane — positions, not ops, are dealt out, so an M op of millions of columns
// is spread over thousands of lanes, and a tile with one op per column costs every lane a walk over its own kCols columns'
// ops.  With P_ref / P_qry the inclusive 64-bit prefixes over the pool (svx_lift.hip's three scan launches, shared), the
// workgroup brackets its ops with two upper bounds among the alignment's P_ref, every lane finds the op of its first
// position by one upper bound inside that bracket and walks forward.  Per lane the kCols reference bytes are one 16-byte
// register load; per run of columns inside one op the SEQ bytes are one more, fetched so that byte c is column c.  Both
// are five aligned dwords and v_alignbyte: the pool offsets have any alignment.  Dwords without a difference under 0xDF
// — all but one in a few hundred — cost one XOR and one AND.
//
// Six launches, nothing handed between workgroups inside one:
//   k_lift_sums, k_lift_chunks, k_lift_apply   P_ref, P_qry (svx_lift_prefixes);
//   k_mismatch<false>   one workgroup per tile: every lane's event count, scanned inside the workgroup: the lane's offset
//                       inside its tile (16 bits) and the tile's count;
//   k_lift_chunks       exclusive scan of the tile counts (svx_lift_exclusive), one entry more than tiles: the total;
//   k_mismatch<true>    the same walk again, every event written at tile base + lane offset + its rank in the lane — rows
//                       at or behind `cap` are not written.
// Count, scan, emit — not slabs: a tile can hold SVX_MISMATCH_TILE events of 14 bytes, a slab per tile would be 28 times
// the bytes the tile reads, to spare a second read of 2 bytes per column.  The order is (alignment, reference position) by
// construction; no atomics.  Every word of the prefixes, the lane offsets, the tile counts and bases and of the 16 + 32
// bytes of padding around the staged pool is written by this call before a launch reads it.
#include "svx_internal.h"
#include "svx_scan_dev.h"

namespace {

constexpr int kThreads = kScanThreads;
constexpr int kCols = SVX_MISMATCH_TILE / kThreads;
static_assert(kCols * kThreads == SVX_MISMATCH_TILE && kCols == 16, "sixteen reference positions per lane: one 16-byte word");
constexpr uint64_t kMaxTiles = 0x7FFFFFFEull;  // gridDim.x, and one entry more for the total
constexpr size_t kPadFront = 16, kPadBack = 32;  // what the 16-byte loads may touch in front of and behind the pool

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

// A C G T among the upper-cased bytes
__device__ __forceinline__ bool is_acgt(uint32_t b) {
    const uint32_t k = b - 0x41u;
    return k < 32u && ((1u << 0 | 1u << 2 | 1u << 6 | 1u << 19) >> k) & 1u;
}

struct Args {
    const uint32_t* cigar;
    const uint64_t* aln_off;
    const int32_t* ref_start;
    const uint64_t* p_ref;
    const uint64_t* p_qry;
    const uint8_t* bases;
    const uint64_t* ref_off;
    const uint32_t* ref_len;
    const uint64_t* qry_off;
    const uint32_t* qry_len;
    const uint64_t* tile_off;  // n_aln + 1
    uint32_t n_aln;
    uint16_t* lane_off;        // kThreads per tile
    svx_use* tile_sum;         // n_tiles + 1
    const svx_use* tile_base;  // n_tiles + 1
    svx_mismatch_soa out;
    uint64_t cap;
};

template <bool EMIT>
__global__ __launch_bounds__(kThreads) void k_mismatch(const Args g) {
    __shared__ uint32_t s_w[kScanWaves];
    const int tid = (int)threadIdx.x;
    const uint64_t t = blockIdx.x;
    // the alignment of tile t: tile_off[a] <= t < tile_off[a + 1]
    const uint32_t a = (uint32_t)upper_bound(g.tile_off, 0, (uint64_t)g.n_aln + 1, t) - 1u;
    const uint64_t tile_r0 = (t - g.tile_off[a]) * SVX_MISMATCH_TILE;  // (< ref_len[a]: the tile exists)
    const uint64_t b = g.aln_off[a], e = g.aln_off[a + 1];
    const uint64_t rlen = g.ref_len[a], qlen = g.qry_len[a];
    uint32_t n = 0;
    uint64_t at = 0;
    if (EMIT) at = g.tile_base[t].ref + g.lane_off[t * kThreads + tid];
    if (e > b && qlen) {
        const uint64_t base_ref = b ? g.p_ref[b - 1] : 0, base_qry = b ? g.p_qry[b - 1] : 0;
        const uint64_t end_ref = g.p_ref[e - 1];
        const uint64_t tile_t0 = base_ref + tile_r0;
        const uint64_t r0 = tile_r0 + (uint64_t)tid * kCols;
        if (tile_t0 < end_ref && r0 < rlen) {
            const uint64_t tile_r1 = tile_r0 + SVX_MISMATCH_TILE < rlen ? tile_r0 + SVX_MISMATCH_TILE : rlen;
            const uint64_t tile_t1 = base_ref + tile_r1 < end_ref ? base_ref + tile_r1 : end_ref;  // (> tile_t0)
            // the tile's ops: [op_lo, op_hi], both inside the alignment
            const uint64_t op_lo = upper_bound(g.p_ref, b, e, tile_t0);
            const uint64_t op_hi = upper_bound(g.p_ref, op_lo, e, tile_t1 - 1);
            const uint64_t t0 = base_ref + r0;
            const uint64_t lane_r1 = r0 + kCols < rlen ? r0 + kCols : rlen;
            const uint64_t t1 = base_ref + lane_r1 < end_ref ? base_ref + lane_r1 : end_ref;
            if (t0 < t1) {
                uint32_t R[4];
                load16(g.bases + g.ref_off[a] + r0, R);
                const uint8_t* __restrict__ seq = g.bases + g.qry_off[a];
                const uint32_t pos0 = (uint32_t)((int64_t)g.ref_start[a] + (int64_t)r0);
                uint64_t i = upper_bound(g.p_ref, op_lo, op_hi + 1, t0);  // (<= op_hi: P_ref[op_hi] > tile_t1 - 1 >= t0)
                uint64_t prev = i > b ? g.p_ref[i - 1] : base_ref;
                uint64_t cur = t0;
                while (cur < t1) {
                    const uint64_t pi = g.p_ref[i];
                    if (pi > cur) {
                        const uint64_t seg_end = pi < t1 ? pi : t1;
                        const uint32_t op = g.cigar[i] & 15u;
                        if (op == 0u || op == 7u || op == 8u) {
                            const uint64_t q = (i > b ? g.p_qry[i - 1] : base_qry) - base_qry + (cur - prev);
                            const int c0 = (int)(cur - t0);
                            int c1 = (int)(seg_end - t0);
                            if (q >= qlen) c1 = c0;
                            else if ((uint64_t)(c1 - c0) > qlen - q) c1 = c0 + (int)(qlen - q);
                            if (c1 > c0) {
                                uint32_t Q[4];
                                load16(seq + q - c0, Q);  // byte c of Q: the base of column c
#pragma unroll
                                for (int d = 0; d < 4; ++d) {
                                    const int lo = c0 - 4 * d > 0 ? c0 - 4 * d : 0, hi = c1 - 4 * d < 4 ? c1 - 4 * d : 4;
                                    if (hi <= lo) continue;
                                    const uint32_t m = (hi == 4 ? 0xFFFFFFFFu : (1u << (8 * hi)) - 1u) & ~((1u << (8 * lo)) - 1u);
                                    const uint32_t x = (R[d] ^ Q[d]) & 0xDFDFDFDFu & m;
                                    if (x == 0) continue;
#pragma unroll
                                    for (int k = 0; k < 4; ++k) {
                                        if (((x >> (8 * k)) & 0xFFu) == 0) continue;
                                        const uint32_t rb = (R[d] >> (8 * k)) & 0xDFu, qb = (Q[d] >> (8 * k)) & 0xDFu;
                                        if (!is_acgt(rb) || !is_acgt(qb)) continue;
                                        if (EMIT) {
                                            const uint64_t row = at + n;
                                            if (row < g.cap) {
                                                const int c = 4 * d + k;
                                                g.out.aln[row] = a;
                                                g.out.ref_pos[row] = pos0 + (uint32_t)c;
                                                g.out.qry_pos[row] = (uint32_t)(q + (uint64_t)(c - c0));
                                                g.out.ref_base[row] = (uint8_t)rb;
                                                g.out.qry_base[row] = (uint8_t)qb;
                                            }
                                        }
                                        ++n;
                                    }
                                }
                            }
                        }
                        cur = seg_end;
                        if (cur < pi) break;  // (cur == t1)
                    }
                    prev = pi;
                    ++i;
                }
            }
        }
    }
    if (!EMIT) {
        uint32_t total;
        const uint32_t before = group_before(wave_scan(n, OpAdd32()), s_w, tid, OpAdd32(), &total);
        g.lane_off[t * kThreads + tid] = (uint16_t)before;  // (<= SVX_MISMATCH_TILE - 1 wherever a lane behind it has events)
        if (tid == 0) {
            g.tile_sum[t] = svx_use{total, 0};
            if (t == 0) g.tile_sum[gridDim.x] = svx_use{0, 0};  // its exclusive sum is the total
        }
    }
}

int mismatch(svx_ctx* ctx, const char* who, const uint32_t* cigar, const uint32_t* d_pool, uint64_t pool_ops, const uint64_t* aln_off,
             const int32_t* ref_start, uint32_t n_aln, const uint8_t* bases, uint64_t n_bases, const uint64_t* ref_off,
             const uint32_t* ref_len, const uint64_t* qry_off, const uint32_t* qry_len, svx_mismatch_soa out, uint64_t cap,
             uint64_t* n_out) {
    if (!ctx) return SVX_E_INVALID;
    if (!n_out || !aln_off) return SVX_E_INVALID;
    *n_out = 0;
    if (n_aln && (!ref_start || !ref_off || !ref_len || !qry_off || !qry_len)) return SVX_E_INVALID;
    if (n_bases && !bases) return SVX_E_INVALID;
    if (cap && (!out.aln || !out.ref_pos || !out.qry_pos || !out.ref_base || !out.qry_base)) return SVX_E_INVALID;
    uint64_t n_ops;
    SVX_TRY(svx_lift_check_offsets(ctx, who, aln_off, n_aln, cigar, d_pool, pool_ops, &n_ops));
    std::vector<uint64_t> tile_off((size_t)n_aln + 1, 0);
    uint64_t most = 0;  // no more events than columns inside both lengths
    for (uint32_t a = 0; a < n_aln; ++a) {
        if (ref_start[a] < 0) {
            SVX_SET_ERR(ctx, "%s: alignment %u starts at %d", who, a, ref_start[a]);
            return SVX_E_INVALID;
        }
        if ((uint64_t)ref_start[a] + ref_len[a] > 0xFFFFFFFFull) {
            SVX_SET_ERR(ctx, "%s: the window of alignment %u ends at %llu, behind 2^32 - 1", who, a,
                        (unsigned long long)((uint64_t)ref_start[a] + ref_len[a]));
            return SVX_E_INVALID;
        }
        if (ref_off[a] > n_bases || ref_len[a] > n_bases - ref_off[a]) {
            SVX_SET_ERR(ctx, "%s: the window of alignment %u ends behind the %llu bases", who, a, (unsigned long long)n_bases);
            return SVX_E_INVALID;
        }
        if (qry_off[a] > n_bases || qry_len[a] > n_bases - qry_off[a]) {
            SVX_SET_ERR(ctx, "%s: the sequence of alignment %u ends behind the %llu bases", who, a, (unsigned long long)n_bases);
            return SVX_E_INVALID;
        }
        const bool walked = ref_len[a] && qry_len[a] && aln_off[a + 1] > aln_off[a];  // (otherwise: no column, no tile)
        tile_off[a + 1] = tile_off[a] + (walked ? ((uint64_t)ref_len[a] + SVX_MISMATCH_TILE - 1) / SVX_MISMATCH_TILE : 0);
        if (walked) most += ref_len[a] < qry_len[a] ? ref_len[a] : qry_len[a];
    }
    const uint64_t n_tiles = tile_off[n_aln];
    if (n_tiles == 0) return SVX_OK;
    const uint64_t n_chunks = (n_ops + SVX_LIFT_CHUNK - 1) / SVX_LIFT_CHUNK;
    if (n_tiles > kMaxTiles || n_chunks > kMaxTiles) {
        SVX_SET_ERR(ctx, "%s: %llu tiles of %d reference positions and %llu ops, at most %llu tiles and %llu ops", who,
                    (unsigned long long)n_tiles, SVX_MISMATCH_TILE, (unsigned long long)n_ops, (unsigned long long)kMaxTiles,
                    (unsigned long long)(kMaxTiles * SVX_LIFT_CHUNK));
        return SVX_E_TOO_LARGE;
    }
    const uint64_t rows = cap < most ? cap : most;  // no more rows are ever written
    SVX_HIP(ctx, hipSetDevice(ctx->device));
    const uint32_t* d_cigar = d_pool;
    uint64_t *d_off, *d_tile_off, *d_ref_off, *d_qry_off, *d_pref, *d_pqry;
    int32_t* d_start;
    uint32_t *d_ref_len, *d_qry_len;
    uint8_t* d_padded;
    svx_mismatch_soa d_out;
    uint16_t* d_lane_off;
    svx_use *d_sum, *d_base, *d_tile_sum, *d_tile_base;
    svx_takes st, ws;
    if (!d_pool) st.add_up(&d_cigar, cigar, n_ops);
    st.add_up(&d_off, aln_off, (size_t)n_aln + 1);
    st.add_up(&d_tile_off, tile_off.data(), (size_t)n_aln + 1);
    st.add_up(&d_ref_off, ref_off, n_aln);
    st.add_up(&d_qry_off, qry_off, n_aln);
    st.add_up(&d_start, ref_start, n_aln);
    st.add_up(&d_ref_len, ref_len, n_aln);
    st.add_up(&d_qry_len, qry_len, n_aln);
    st.add(&d_padded, kPadFront + n_bases + kPadBack);
    st.add(&d_out.aln, rows);
    st.add(&d_out.ref_pos, rows);
    st.add(&d_out.qry_pos, rows);
    st.add(&d_out.ref_base, rows);
    st.add(&d_out.qry_base, rows);
    ws.add(&d_pref, n_ops);
    ws.add(&d_pqry, n_ops);
    ws.add(&d_sum, n_chunks);
    ws.add(&d_base, n_chunks);
    ws.add(&d_lane_off, n_tiles * kThreads);
    ws.add(&d_tile_sum, n_tiles + 1);
    ws.add(&d_tile_base, n_tiles + 1);
    SVX_TRY(svx_stage_lay(ctx, st));
    SVX_TRY(svx_ws_lay(ctx, ws));
    // (the loads never use a padding byte, but they fetch it: written like every other word)
    SVX_HIP(ctx, hipMemsetAsync(d_padded, 0, kPadFront, ctx->stream));
    SVX_TRY(svx_upload(ctx, d_padded + kPadFront, bases, n_bases));
    SVX_HIP(ctx, hipMemsetAsync(d_padded + kPadFront + n_bases, 0, kPadBack, ctx->stream));
    SVX_TRY(svx_timing_begin(ctx));
    SVX_TRY(svx_lift_prefixes(ctx, d_cigar, n_ops, d_sum, d_base, d_pref, d_pqry));
    SVX_TRY(svx_timing_mark(ctx, 1));
    Args g;
    g.cigar = d_cigar;
    g.aln_off = d_off;
    g.ref_start = d_start;
    g.p_ref = d_pref;
    g.p_qry = d_pqry;
    g.bases = d_padded + kPadFront;
    g.ref_off = d_ref_off;
    g.ref_len = d_ref_len;
    g.qry_off = d_qry_off;
    g.qry_len = d_qry_len;
    g.tile_off = d_tile_off;
    g.n_aln = n_aln;
    g.lane_off = d_lane_off;
    g.tile_sum = d_tile_sum;
    g.tile_base = d_tile_base;
    g.out = d_out;
    g.cap = rows;
    hipLaunchKernelGGL(k_mismatch<false>, dim3((uint32_t)n_tiles), dim3(kThreads), 0, ctx->stream, g);
    SVX_HIP(ctx, hipGetLastError());
    SVX_TRY(svx_lift_exclusive(ctx, d_tile_sum, (uint32_t)n_tiles + 1, d_tile_base));
    hipLaunchKernelGGL(k_mismatch<true>, dim3((uint32_t)n_tiles), dim3(kThreads), 0, ctx->stream, g);
    SVX_HIP(ctx, hipGetLastError());
    SVX_TRY(svx_timing_mark(ctx, 2));
    SVX_TRY(svx_timing_end(ctx));
    svx_use total;
    SVX_TRY(svx_download(ctx, &total, d_tile_base + n_tiles, 1));
    SVX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *n_out = total.ref;
    const uint64_t k = total.ref < cap ? total.ref : cap;  // (<= rows: total <= most)
    if (k) {
        SVX_TRY(svx_download(ctx, out.aln, d_out.aln, k));
        SVX_TRY(svx_download(ctx, out.ref_pos, d_out.ref_pos, k));
        SVX_TRY(svx_download(ctx, out.qry_pos, d_out.qry_pos, k));
        SVX_TRY(svx_download(ctx, out.ref_base, d_out.ref_base, k));
        SVX_TRY(svx_download(ctx, out.qry_base, d_out.qry_base, k));
        SVX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    return total.ref > cap ? SVX_E_CAPACITY : SVX_OK;
}

}  // namespace

extern "C" int svx_cigar_mismatch(svx_ctx* ctx, const uint32_t* cigar, const uint64_t* aln_off, const int32_t* ref_start, uint32_t n_aln,
                                  const uint8_t* bases, uint64_t n_bases, const uint64_t* ref_off, const uint32_t* ref_len,
                                  const uint64_t* qry_off, const uint32_t* qry_len, svx_mismatch_soa out, uint64_t cap, uint64_t* n_out) {
    return mismatch(ctx, "svx_cigar_mismatch", cigar, nullptr, 0, aln_off, ref_start, n_aln, bases, n_bases, ref_off, ref_len, qry_off,
                    qry_len, out, cap, n_out);
}

extern "C" int svx_cigar_mismatch_dev(svx_ctx* ctx, const uint32_t* d_cigar, uint64_t n_ops, const uint64_t* aln_off,
                                      const int32_t* ref_start, uint32_t n_aln, const uint8_t* bases, uint64_t n_bases,
                                      const uint64_t* ref_off, const uint32_t* ref_len, const uint64_t* qry_off, const uint32_t* qry_len,
                                      svx_mismatch_soa out, uint64_t cap, uint64_t* n_out) {
    if (!d_cigar && n_ops) return SVX_E_INVALID;
    return mismatch(ctx, "svx_cigar_mismatch_dev", nullptr, d_cigar, n_ops, aln_off, ref_start, n_aln, bases, n_bases, ref_off, ref_len,
                    qry_off, qry_len, out, cap, n_out);
}
