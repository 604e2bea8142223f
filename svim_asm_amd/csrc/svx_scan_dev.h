// svx_scan_dev.h — the wave and workgroup scan ladder of svx_cover.hip and svx_lift.hip (gfx9 family DPP), for any value
// type made of 32-bit words whose all-zero pattern is the operator's identity: unsigned maxima, sums, pairs of them.
// Workgroups of kScanThreads lanes.  Device code only; every translation unit that includes it gets its own copy.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

namespace {

constexpr int kScanThreads = 256;
constexpr int kScanWaves = kScanThreads / 64;

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
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint64_t dpp0_64(uint64_t v) { return dpp0<CTRL, ROW_MASK>(v); }
__device__ __forceinline__ uint64_t max64(uint64_t a, uint64_t b) { return a > b ? a : b; }
__device__ __forceinline__ uint64_t min64(uint64_t a, uint64_t b) { return a < b ? a : b; }
struct OpMax {
    __device__ __forceinline__ uint64_t operator()(uint64_t a, uint64_t b) const { return max64(a, b); }
};
struct OpAdd {
    __device__ __forceinline__ uint64_t operator()(uint64_t a, uint64_t b) const { return a + b; }
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

}  // namespace
