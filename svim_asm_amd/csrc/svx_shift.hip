// svx_shift.hip — "how far to the left can this small gap move without changing the haplotype?" for a batch of insertions
// and deletions on gfx950 (svx_indel_shift, include/svx.h).
//
// The definition is the loop in include/svx.h.  Step i passes the aligned column (ref[r - i], qry[q - i]) and needs, for the
// gap to stay the same edit, the base X that leaves the gap's right end to equal the base that enters at its left end.  The
// index conditions of the loop hold for every step once they hold for step 1 and i <= min(r, q), so the walk has a closed
// bound on its steps — min(ev_limit, r, q), or 0 where step 1 is already outside a range — and what is left is a run of byte
// compares downwards from three addresses: ref + r, qry + q and the right end (qry + q + L or ref + r + L).
//
// Nearly every event stops within a handful of steps; a microsatellite or a long homopolymer runs for hundreds to thousands,
// and one such lane would stall its wave.  Two forms with identical outputs:
//   k_shift_lane    one lane per event, at most `lane_steps` steps, a byte per step and stream.  shift[e] = the steps taken;
//                   an event that still matches with steps left under its bound is UNDECIDED: its index goes to its
//                   workgroup's part of `local` at its rank among the workgroup's undecided lanes (wave_scan /
//                   group_before), and the workgroup's count to `count`;
//   k_shift_bases   one workgroup's exclusive sum of the counts (carried_scan), one entry more than workgroups: the total,
//                   which the host reads back;
//   k_shift_list    every workgroup's part of `local` to its place in the dense list: event order, no atomics;
//   k_shift_wave    one wave per listed event, from shift[e] on: per iteration SVX_SHIFT_WAVE_COLS consecutive steps, four
//                   per lane — one unaligned dword from each of the three streams as two aligned dwords and v_alignbyte: the
//                   pool offsets have any alignment —, a step behind the bound counting as failing; one __ballot of the
//                   lanes with a failing step, and the lowest failing step ends the walk.
// The host waits for the total between k_shift_list and k_shift_wave and launches exactly that many waves, none for zero —
// the usual case with the default hand-over (DESIGN §3.19 has the reasons).  Every word of the counts, the bases, the parts
// of `local` that are read, the list and of the 16 + 32 bytes of padding around the staged pool is written by this call
// before a launch reads it.
#include "svx_internal.h"
#include "svx_scan_dev.h"

namespace {

constexpr int kThreads = kScanThreads;
constexpr int kPer = SVX_SHIFT_WAVE_COLS / 64;  // steps of one lane per iteration of the wave form
static_assert(kPer == 4 && kPer * 64 == SVX_SHIFT_WAVE_COLS, "one dword of each stream per lane");
constexpr uint64_t kMaxEvents = 0x7FFFFF00ull;   // gridDim.x of the wave form at four events per workgroup and of the lane form
constexpr size_t kPadFront = 16, kPadBack = 32;  // what the dword loads may touch in front of and behind the pool

struct Args {
    const uint8_t* bases;
    const uint64_t* ref_off;
    const uint32_t* ref_len;
    const uint64_t* qry_off;
    const uint32_t* qry_len;
    const int32_t* ref_start;
    const uint32_t* ev_aln;
    const uint32_t* ev_ref_pos;
    const uint32_t* ev_qry_pos;
    const uint32_t* ev_len;
    const uint8_t* ev_type;
    const uint32_t* ev_limit;
    uint32_t n_ev;
    uint32_t lane_steps;
    uint32_t* shift;
    uint32_t* local;   // kThreads per workgroup of the lane form
    uint32_t* count;   // workgroups + 1
    uint32_t* base;    // workgroups + 1
    uint32_t* list;    // n_ev
    uint32_t n_list;   // (the wave form only)
};

// A C G T among the upper-cased bytes
__device__ __forceinline__ bool is_acgt(uint32_t b) {
    const uint32_t k = b - 0x41u;
    return k < 32u && ((1u << 0 | 1u << 2 | 1u << 6 | 1u << 19) >> k) & 1u;
}

// the 4 bytes at p (any alignment), little endian: two aligned dwords, v_alignbyte
__device__ __forceinline__ uint32_t load4(const uint8_t* __restrict__ p) {
    const uint32_t sh = (uint32_t)((uintptr_t)p & 3u);
    const uint32_t* __restrict__ w = reinterpret_cast<const uint32_t*>((uintptr_t)p & ~(uintptr_t)3);
    return __builtin_amdgcn_alignbyte(w[1], w[0], sh);
}

// One event's walk: step i compares r_end[-i], q_end[-i] and x_end[-i], i = 1 .. bound.
struct Walk {
    const uint8_t* r_end;  // ref + r
    const uint8_t* q_end;  // qry + q
    const uint8_t* x_end;  // the gap's right end: qry + q + L (INS) or ref + r + L (DEL)
    uint32_t bound;        // the most steps the limit and the ranges allow
};

__device__ __forceinline__ Walk walk_of(const Args& g, uint32_t e) {
    const uint32_t a = g.ev_aln[e];
    const uint64_t r = (uint64_t)((int64_t)g.ev_ref_pos[e] - (int64_t)g.ref_start[a]);  // (>= 0: checked on the host)
    const uint64_t q = g.ev_qry_pos[e], len = g.ev_len[e];
    const uint64_t rlen = g.ref_len[a], qlen = g.qry_len[a];
    const bool ins = g.ev_type[e] == SVX_SIG_INS;
    const uint8_t* ref = g.bases + g.ref_off[a];
    const uint8_t* qry = g.bases + g.qry_off[a];
    Walk w;
    w.r_end = ref + r;
    w.q_end = qry + q;
    w.x_end = ins ? qry + q + len : ref + r + len;
    // step 1 inside both ranges and the right end inside its own: then so is every step up to min(r, q)
    const bool inside = r <= rlen && q <= qlen && (ins ? q + len <= qlen : r + len <= rlen);
    uint64_t b = g.ev_limit[e];
    b = b < r ? b : r;
    b = b < q ? b : q;
    w.bound = inside ? (uint32_t)b : 0u;
    return w;
}

__device__ __forceinline__ bool step_ok(uint32_t R, uint32_t Q, uint32_t X) {
    R &= 0xDFu;
    return is_acgt(R) && R == (Q & 0xDFu) && R == (X & 0xDFu);
}

__global__ __launch_bounds__(kThreads) void k_shift_lane(const Args g) {
    __shared__ uint32_t s_w[kScanWaves];
    const int tid = (int)threadIdx.x;
    const uint64_t e64 = (uint64_t)blockIdx.x * kThreads + (uint64_t)tid;
    uint32_t undecided = 0;
    if (e64 < g.n_ev) {
        const uint32_t e = (uint32_t)e64;
        const Walk w = walk_of(g, e);
        const uint32_t most = w.bound < g.lane_steps ? w.bound : g.lane_steps;
        uint32_t k = 0;
        while (k < most && step_ok(w.r_end[-(int64_t)(k + 1)], w.q_end[-(int64_t)(k + 1)], w.x_end[-(int64_t)(k + 1)])) ++k;
        g.shift[e] = k;
        undecided = k == most && most < w.bound ? 1u : 0u;
    }
    uint32_t total;
    const uint32_t before = group_before(wave_scan(undecided, OpAdd32()), s_w, tid, OpAdd32(), &total);
    if (undecided) g.local[(uint64_t)blockIdx.x * kThreads + before] = (uint32_t)e64;
    if (tid == 0) {
        g.count[blockIdx.x] = total;
        if (blockIdx.x == 0) g.count[gridDim.x] = 0;  // its exclusive sum is the total
    }
}

__global__ __launch_bounds__(kThreads) void k_shift_bases(const uint32_t* __restrict__ count, uint32_t n, uint32_t* __restrict__ base) {
    __shared__ uint32_t s_wave[2][kScanWaves];
    carried_scan<uint32_t>(0, n, OpAdd32(), [&](uint64_t i) { return count[i]; },
                           [&](uint64_t i, uint32_t before, uint32_t) { base[i] = before; }, s_wave);
}

__global__ __launch_bounds__(kThreads) void k_shift_list(const Args g) {
    const uint32_t b = blockIdx.x, tid = threadIdx.x;
    if (tid < g.count[b]) g.list[g.base[b] + tid] = g.local[(uint64_t)b * kThreads + tid];
}

__global__ __launch_bounds__(kThreads) void k_shift_wave(const Args g) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t w64 = (uint64_t)blockIdx.x * kScanWaves + (threadIdx.x >> 6);
    if (w64 >= g.n_list) return;  // (the whole wave)
    const uint32_t e = g.list[w64];
    const Walk w = walk_of(g, e);
    uint32_t k = g.shift[e];  // (< bound: the event is undecided)
    while (k < w.bound) {
        // this lane's steps i0 .. i0 + kPer - 1; step i0 + j is byte kPer - 1 - j of the dword at end - (i0 + kPer - 1)
        const uint64_t i0 = (uint64_t)k + 1 + (uint64_t)lane * kPer;
        uint32_t bad = kPer;  // the lane's first failing step, as j
        if (i0 > w.bound) {
            bad = 0;  // (nothing is loaded: the dword could lie in front of the range by more than the padding)
        } else {
            const int64_t back = -(int64_t)(i0 + kPer - 1);
            const uint32_t R = load4(w.r_end + back), Q = load4(w.q_end + back), X = load4(w.x_end + back);
#pragma unroll
            for (int j = kPer - 1; j >= 0; --j) {
                const int s = 8 * (kPer - 1 - j);
                if (i0 + j > w.bound || !step_ok(R >> s & 0xFFu, Q >> s & 0xFFu, X >> s & 0xFFu)) bad = (uint32_t)j;
            }
        }
        const uint64_t failing = __ballot(bad < (uint32_t)kPer);
        if (failing == 0) {
            k += SVX_SHIFT_WAVE_COLS;  // (<= bound: a step behind the bound would have failed)
            continue;
        }
        const int first = __ffsll((long long)failing) - 1;
        k += (uint32_t)first * kPer + (uint32_t)__shfl((int)bad, first);  // the steps in front of the lowest failing one
        break;
    }
    if (lane == 0) g.shift[e] = k;
}

}  // namespace

extern "C" int svx_ctx_set_shift_lane_steps(svx_ctx* ctx, int32_t steps) {
    if (!ctx) return SVX_E_INVALID;
    ctx->shift_lane_steps = steps;  // (negative: the default, resolved where the call plans its launches)
    return SVX_OK;
}

extern "C" int svx_indel_shift(svx_ctx* ctx, const uint8_t* bases, uint64_t n_bases, const uint64_t* ref_off, const uint32_t* ref_len,
                               const uint64_t* qry_off, const uint32_t* qry_len, const int32_t* ref_start, uint32_t n_aln,
                               const uint32_t* ev_aln, const uint32_t* ev_ref_pos, const uint32_t* ev_qry_pos, const uint32_t* ev_len,
                               const uint8_t* ev_type, const uint32_t* ev_limit, uint32_t n_ev, uint32_t* shift) {
    const char* who = "svx_indel_shift";
    if (!ctx) return SVX_E_INVALID;
    if (n_aln && (!ref_off || !ref_len || !qry_off || !qry_len || !ref_start)) return SVX_E_INVALID;
    if (n_ev && (!ev_aln || !ev_ref_pos || !ev_qry_pos || !ev_len || !ev_type || !ev_limit || !shift)) return SVX_E_INVALID;
    if (n_bases && !bases) return SVX_E_INVALID;
    for (uint32_t a = 0; a < n_aln; ++a) {
        if (ref_start[a] < 0) {
            SVX_SET_ERR(ctx, "%s: alignment %u starts at %d", who, a, ref_start[a]);
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
    }
    for (uint32_t e = 0; e < n_ev; ++e) {
        if (ev_aln[e] >= n_aln) {
            SVX_SET_ERR(ctx, "%s: event %u names alignment %u of %u", who, e, ev_aln[e], n_aln);
            return SVX_E_INVALID;
        }
        if ((int64_t)ev_ref_pos[e] < (int64_t)ref_start[ev_aln[e]]) {
            SVX_SET_ERR(ctx, "%s: event %u lies at %u, in front of its alignment's start %d", who, e, ev_ref_pos[e], ref_start[ev_aln[e]]);
            return SVX_E_INVALID;
        }
        if (ev_type[e] != SVX_SIG_INS && ev_type[e] != SVX_SIG_DEL) {
            SVX_SET_ERR(ctx, "%s: event %u has type %u, neither SVX_SIG_INS nor SVX_SIG_DEL", who, e, (unsigned)ev_type[e]);
            return SVX_E_INVALID;
        }
        if (ev_len[e] == 0) {
            SVX_SET_ERR(ctx, "%s: event %u has length 0", who, e);
            return SVX_E_INVALID;
        }
    }
    if (n_ev == 0) return SVX_OK;
    if (n_ev > kMaxEvents) {
        SVX_SET_ERR(ctx, "%s: %u events, at most %llu", who, n_ev, (unsigned long long)kMaxEvents);
        return SVX_E_TOO_LARGE;
    }
    const uint32_t n_groups = (n_ev + kThreads - 1) / kThreads;
    SVX_HIP(ctx, hipSetDevice(ctx->device));
    uint8_t* d_padded;
    Args g;
    svx_takes st, ws;
    st.add_up(&g.ref_off, ref_off, n_aln);
    st.add_up(&g.ref_len, ref_len, n_aln);
    st.add_up(&g.qry_off, qry_off, n_aln);
    st.add_up(&g.qry_len, qry_len, n_aln);
    st.add_up(&g.ref_start, ref_start, n_aln);
    st.add_up(&g.ev_aln, ev_aln, n_ev);
    st.add_up(&g.ev_ref_pos, ev_ref_pos, n_ev);
    st.add_up(&g.ev_qry_pos, ev_qry_pos, n_ev);
    st.add_up(&g.ev_len, ev_len, n_ev);
    st.add_up(&g.ev_type, ev_type, n_ev);
    st.add_up(&g.ev_limit, ev_limit, n_ev);
    st.add(&d_padded, kPadFront + n_bases + kPadBack);
    st.add(&g.shift, n_ev);
    ws.add(&g.local, (size_t)n_groups * kThreads);
    ws.add(&g.count, (size_t)n_groups + 1);
    ws.add(&g.base, (size_t)n_groups + 1);
    ws.add(&g.list, n_ev);
    SVX_TRY(svx_stage_lay(ctx, st));
    SVX_TRY(svx_ws_lay(ctx, ws));
    // (the loads never use a padding byte, but they fetch it: written like every other word)
    SVX_HIP(ctx, hipMemsetAsync(d_padded, 0, kPadFront, ctx->stream));
    SVX_TRY(svx_upload(ctx, d_padded + kPadFront, bases, n_bases));
    SVX_HIP(ctx, hipMemsetAsync(d_padded + kPadFront + n_bases, 0, kPadBack, ctx->stream));
    g.bases = d_padded + kPadFront;
    g.n_ev = n_ev;
    const int32_t steps = ctx->shift_lane_steps < 0 ? SVX_SHIFT_LANE_STEPS : ctx->shift_lane_steps;
    g.lane_steps = steps == INT32_MAX ? 0xFFFFFFFFu : (uint32_t)steps;
    g.n_list = 0;
    SVX_TRY(svx_timing_begin(ctx));
    hipLaunchKernelGGL(k_shift_lane, dim3(n_groups), dim3(kThreads), 0, ctx->stream, g);
    SVX_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_shift_bases, dim3(1), dim3(kThreads), 0, ctx->stream, (const uint32_t*)g.count, n_groups + 1, g.base);
    SVX_HIP(ctx, hipGetLastError());
    uint32_t n_list = 0;
    SVX_TRY(svx_download(ctx, &n_list, (const uint32_t*)(g.base + n_groups), 1));
    hipLaunchKernelGGL(k_shift_list, dim3(n_groups), dim3(kThreads), 0, ctx->stream, g);
    SVX_HIP(ctx, hipGetLastError());
    SVX_TRY(svx_timing_mark(ctx, 1));
    SVX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (n_list) {  // (<= n_ev)
        g.n_list = n_list;
        hipLaunchKernelGGL(k_shift_wave, dim3((n_list + kScanWaves - 1) / kScanWaves), dim3(kThreads), 0, ctx->stream, g);
        SVX_HIP(ctx, hipGetLastError());
    }
    SVX_TRY(svx_timing_mark(ctx, 2));
    SVX_TRY(svx_timing_end(ctx));
    SVX_TRY(svx_download(ctx, shift, (const uint32_t*)g.shift, n_ev));
    SVX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SVX_OK;
}
