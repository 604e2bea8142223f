// svx_scan_dev.h — the one place for scan and search on the device (gfx9 family DPP): the wave scan ladder, one workgroup's
// single-pass prefix (group_before) and its chunked, carried scan over any range (carried_scan), for any value type made
// of 32-bit words whose all-zero pattern is the operator's identity — unsigned maxima, sums, pairs of them —, and the
// upper bound among sorted 64- or 32-bit keys.  Workgroups of kScanThreads lanes.  Device code only; every translation unit that
// includes it gets its own copy.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

namespace {

constexpr int kScanThreads = 256;
constexpr int kScanWaves = kScanThreads / 64;
constexpr int kScanPer = 4;                           // consecutive elements of one lane
constexpr int kScanChunk = kScanThreads * kScanPer;   // elements of one pass of carried_scan

// DPP lane movement: 0 flows into lanes without a source — the identity of max over unsigned keys, of the sum, and (word
// by word) of every pair or tuple of them
template <int CTRL, int ROW_MASK, typename T>
__device__ __forceinline__ T dpp0(T v) {
    static_assert(sizeof(T) % 4 == 0, "whole 32-bit words");
    uint32_t w[sizeof(T) / 4];
    memcpy(w, &v, sizeof(T));
#pragma unroll
    for (size_t k = 0; k < sizeof(T) / 4; ++k) w[k] = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)w[k], CTRL, ROW_MASK, 0xF, false);
    memcpy(&v, w, sizeof(T));
    return v;
}
__device__ __forceinline__ uint64_t max64(uint64_t a, uint64_t b) { return a > b ? a : b; }
__device__ __forceinline__ uint64_t min64(uint64_t a, uint64_t b) { return a < b ? a : b; }
struct OpMax {
    __device__ __forceinline__ uint64_t operator()(uint64_t a, uint64_t b) const { return max64(a, b); }
};
struct OpAdd {
    __device__ __forceinline__ uint64_t operator()(uint64_t a, uint64_t b) const { return a + b; }
};
struct OpAdd32 {
    __device__ __forceinline__ uint32_t operator()(uint32_t a, uint32_t b) const { return a + b; }
};
// inclusive scan over the lanes 0..l of the wave; 0 is op's identity.  Every step combines two DISJOINT lane ranges
// (row_shr:n the n lanes in front of the 2^k a lane holds, row_bcast the whole rows in front), rows a step's mask leaves
// out and lanes without a source combine with 0: op need not be idempotent.
template <typename T, typename Op>
__device__ __forceinline__ T wave_scan(T v, Op op) {
    v = op(v, dpp0<0x111, 0xF>(v));  // row_shr:1
    v = op(v, dpp0<0x112, 0xF>(v));  // row_shr:2
    v = op(v, dpp0<0x114, 0xF>(v));  // row_shr:4
    v = op(v, dpp0<0x118, 0xF>(v));  // row_shr:8
    v = op(v, dpp0<0x142, 0xA>(v));  // row_bcast:15 into rows 1 and 3
    v = op(v, dpp0<0x143, 0xC>(v));  // row_bcast:31 into rows 2 and 3
    return v;
}

// Exclusive prefix of a lane's inclusive wave scan `incl` over the whole workgroup: the lanes in front of it in its wave
// (wave_shr:1, lane 0 receives 0), the waves in front through `s_w`, and `total` of all four waves.  One barrier; the
// caller keeps a second one between two uses of the same `s_w`.
template <typename T, typename Op>
__device__ __forceinline__ T group_before(T incl, T* s_w, int tid, Op op, T* total) {
    const int wave = tid >> 6;
    if ((tid & 63) == 63) s_w[wave] = incl;
    T before = dpp0<0x138, 0xF>(incl);
    __syncthreads();
    T all = s_w[0];
#pragma unroll
    for (int w = 1; w < kScanWaves; ++w) {
        if (w == wave) before = op(before, all);  // (waves 0..w-1, disjoint from this wave's lanes)
        all = op(all, s_w[w]);
    }
    *total = all;
    return before;
}

// One workgroup's inclusive scan of the elements [lo, hi) under op, kScanChunk of them per pass: kScanPer consecutive
// elements per lane scanned in registers, wave_scan of the lanes' last ones, the four waves folded through LDS, the running
// value carried from pass to pass.  load(i) gives element i and store(i, before, incl) takes its exclusive and inclusive
// prefix; both are called for lo <= i < hi only — elements at or behind hi count as T{}, and nothing outside [lo, hi) is
// stored, whatever the memory behind it held.
//  * The trip count depends on lo and hi alone, which are the same for the whole workgroup: every lane takes every pass,
//    its DPP steps and its barrier included.
//  * Every combine is over disjoint ranges of elements (a lane's earlier elements, the lanes in front, the waves in front,
//    the passes in front): op need not be idempotent.
//  * s_wave's two buffers are used in turn with ONE barrier per pass: a buffer's next write is behind the next pass's
//    barrier, which every lane reaches only after its reads of this pass.
template <typename T, typename Op, typename Load, typename Store>
__device__ __forceinline__ void carried_scan(uint64_t lo, uint64_t hi, Op op, Load load, Store store, T (*s_wave)[kScanWaves]) {
    const int tid = (int)threadIdx.x, wave = tid >> 6;
    T carry{};
    int slot = 0;
    for (uint64_t base = lo; base < hi; base += kScanChunk, slot ^= 1) {
        const uint64_t first = base + (uint64_t)tid * kScanPer;
        T v[kScanPer];
#pragma unroll
        for (int j = 0; j < kScanPer; ++j) v[j] = first + j < hi ? load(first + j) : T{};
#pragma unroll
        for (int j = 1; j < kScanPer; ++j) v[j] = op(v[j - 1], v[j]);
        const T incl = wave_scan(v[kScanPer - 1], op);
        if ((tid & 63) == 63) s_wave[slot][wave] = incl;
        T before = dpp0<0x138, 0xF>(incl);  // the lanes in front of this one: wave_shr:1, lane 0 receives 0
        __syncthreads();
        T total{};
#pragma unroll
        for (int w = 0; w < kScanWaves; ++w) {
            const T t = s_wave[slot][w];
            if (w < wave) before = op(before, t);
            total = op(total, t);
        }
        before = op(carry, before);
#pragma unroll
        for (int j = 0; j < kScanPer; ++j)
            if (first + j < hi) store(first + j, j ? op(before, v[j - 1]) : before, op(before, v[j]));
        carry = op(carry, total);
    }
}

// first index in [lo, hi) with p[index] > target, hi when there is none (keys of 64 or of 32 bits)
template <typename K>
__device__ __forceinline__ uint64_t upper_bound(const K* __restrict__ p, uint64_t lo, uint64_t hi, uint64_t target) {
    uint64_t n = hi - lo;
    while (n) {
        const uint64_t half = n >> 1;
        if (p[lo + half] <= target) { lo += half + 1; n -= half + 1; } else n = half;
    }
    return lo;
}

}  // namespace
