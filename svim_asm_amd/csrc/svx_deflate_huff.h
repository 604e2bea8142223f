// svx_deflate_huff.h — the Huffman side of svx_deflate.hip's dynamic blocks (RFC 1951 §3.2.2, §3.2.7), each routine the
// work of ONE thread: code lengths under a limit, canonical codes, the run-length form of the two length arrays.  Plain
// C++ over caller memory (LDS in the kernel), so the same text compiles for the host: tests/native/deflate_huff.cpp
// drives it with frequency vectors that the device's LZ77 would only produce by luck.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SVX_HUFF_FN static __host__ __device__
#else
#define SVX_HUFF_FN static
#endif

// Huffman work areas, laid over the hash table once the parse is through
struct HuffWork {
    uint32_t key[288];
    uint32_t w[576];
    uint32_t par[576];
    uint32_t blc[16];
};

// Code lengths (<= maxbits) of a tree over n symbols with frequencies f, by one thread.  At least two codes: with fewer
// used symbols, symbols 0 / 1 get length 1 (zlib's rule).  Lengths whose Kraft sum is exactly 1.
SVX_HUFF_FN void build_lengths(const uint32_t* f, int n, int maxbits, uint8_t* len, HuffWork& hw) {
    int m = 0;
    for (int i = 0; i < n; ++i) {
        len[i] = 0;
        if (f[i]) hw.key[m++] = (uint32_t)i;
    }
    if (m < 2) {
        if (m == 0) { len[0] = 1; len[1] = 1; }
        else { len[hw.key[0]] = 1; len[hw.key[0] == 0 ? 1 : 0] = 1; }
        return;
    }
    // ascending (frequency, symbol): insertion sort (<= 286 symbols)
    for (int i = 1; i < m; ++i) {
        const uint32_t k = hw.key[i], fk = f[k];
        int j = i - 1;
        while (j >= 0 && (f[hw.key[j]] > fk || (f[hw.key[j]] == fk && hw.key[j] > k))) {
            hw.key[j + 1] = hw.key[j];
            --j;
        }
        hw.key[j + 1] = k;
    }
    // two queues: leaves 0..m-1 (sorted), internal nodes m.. in creation order (weights never decrease)
    for (int i = 0; i < m; ++i) hw.w[i] = f[hw.key[i]];
    int li = 0, ii = m, next = m;
    for (int k = 0; k < m - 1; ++k) {
        int a, b;
        if (li < m && (ii >= next || hw.w[li] <= hw.w[ii])) a = li++; else a = ii++;
        if (li < m && (ii >= next || hw.w[li] <= hw.w[ii])) b = li++; else b = ii++;
        hw.w[next] = hw.w[a] + hw.w[b];
        hw.par[a] = (uint32_t)next;
        hw.par[b] = (uint32_t)next;
        ++next;
    }
    // depths (reuse w): root = next - 1
    hw.w[next - 1] = 0;
    for (int i = next - 2; i >= 0; --i) hw.w[i] = hw.w[hw.par[i]] + 1u;
    for (int b = 0; b <= 15; ++b) hw.blc[b] = 0;
    for (int i = 0; i < m; ++i) hw.blc[hw.w[i] > (uint32_t)maxbits ? maxbits : hw.w[i]]++;
    // Kraft sum in units of 2^-maxbits
    uint32_t kraft = 0;
    const uint32_t full = 1u << maxbits;
    for (int b = 1; b <= maxbits; ++b) kraft += hw.blc[b] << (maxbits - b);
    while (kraft > full) {  // lengthen a code of the deepest length below maxbits
        int b = maxbits - 1;
        while (hw.blc[b] == 0) --b;
        hw.blc[b]--;
        hw.blc[b + 1]++;
        kraft -= 1u << (maxbits - b - 1);
    }
    while (kraft < full) {  // shorten a code of the deepest length: the smallest step
        int b = maxbits;
        while (hw.blc[b] == 0) --b;
        hw.blc[b]--;
        hw.blc[b - 1]++;
        kraft += 1u << (maxbits - b);
    }
    // the longest codes to the rarest symbols
    int at = 0;
    for (int b = maxbits; b >= 1; --b)
        for (uint32_t c = 0; c < hw.blc[b]; ++c) len[hw.key[at++]] = (uint8_t)b;
}

#if defined(__has_builtin)
#if __has_builtin(__builtin_bitreverse32)
#define SVX_HUFF_HAS_BITREVERSE 1
#endif
#endif
SVX_HUFF_FN uint32_t svx_bitreverse32(uint32_t v) {
#ifdef SVX_HUFF_HAS_BITREVERSE
    return __builtin_bitreverse32(v);
#else
    v = (v >> 1 & 0x55555555u) | (v & 0x55555555u) << 1;
    v = (v >> 2 & 0x33333333u) | (v & 0x33333333u) << 2;
    v = (v >> 4 & 0x0F0F0F0Fu) | (v & 0x0F0F0F0Fu) << 4;
    v = (v >> 8 & 0x00FF00FFu) | (v & 0x00FF00FFu) << 8;
    return v >> 16 | v << 16;
#endif
}

// canonical codes, bit-reversed for the LSB-first stream
SVX_HUFF_FN void make_codes(const uint8_t* len, int n, uint16_t* code) {
    uint32_t cnt[16] = {0}, nxt[16];
    for (int i = 0; i < n; ++i) cnt[len[i]]++;
    cnt[0] = 0;
    uint32_t c = 0;
    for (int b = 1; b <= 15; ++b) {
        c = (c + cnt[b - 1]) << 1;
        nxt[b] = c;
    }
    for (int i = 0; i < n; ++i) {
        const uint32_t l = len[i];
        if (!l) { code[i] = 0; continue; }
        const uint32_t v = nxt[l]++;
        code[i] = (uint16_t)(svx_bitreverse32(v) >> (32 - l));
    }
}

// run-length form of the lengths, HLIT then HDIST back to back (runs may cross: RFC 1951 §3.2.7): code-length symbols
// sym | extra << 8 into rle (room for hlit + hdist entries), their number returned
SVX_HUFF_FN uint32_t rle_lengths(const uint8_t* lit_len, uint32_t hlit, const uint8_t* dist_len, uint32_t hdist, uint16_t* rle) {
    const uint32_t total = hlit + hdist;
    auto L = [&](uint32_t i) -> uint32_t { return i < hlit ? lit_len[i] : dist_len[i - hlit]; };
    uint32_t nr = 0, i = 0;
    while (i < total) {
        const uint32_t v = L(i);
        uint32_t run = 1;
        while (i + run < total && L(i + run) == v) ++run;
        if (v == 0) {
            uint32_t left = run;
            while (left >= 11) { const uint32_t r = left < 138 ? left : 138; rle[nr++] = (uint16_t)(18 | (r - 11) << 8); left -= r; }
            if (left >= 3) { rle[nr++] = (uint16_t)(17 | (left - 3) << 8); left = 0; }
            while (left) { rle[nr++] = 0; --left; }
        } else {
            rle[nr++] = (uint16_t)v;
            uint32_t left = run - 1;
            while (left >= 3) { const uint32_t r = left < 6 ? left : 6; rle[nr++] = (uint16_t)(16 | (r - 3) << 8); left -= r; }
            while (left) { rle[nr++] = (uint16_t)v; --left; }
        }
        i += run;
    }
    return nr;
}
