// svx_deflate.hip — BGZF compression on gfx950: the counterpart of svx_inflate.hip, for `--bgzip_output` (the VCF as
// bgzip writes it).  What it stands in for: `bgzip variants.vcf` (htslib bgzf_write, zlib deflate level 6).
//
// One workgroup (4 waves) per BGZF block of 65 280 input bytes, the block staged in LDS:
//   1. CRC-32 of the block: 64 lanes of wave 0 take 1 KiB each, folded with crc32_combine's operators (as
//      k_inflate_resolve checks it).
//   2. LZ77 over the block, 256 positions at a time (a thread each): candidates are the distances 1-4, the four nearest
//      earlier positions of the same 3-byte hash inside the chunk, and the four most recent ones of earlier chunks (a
//      ring per bucket, filled behind every chunk with the LAST position of the chunk per bucket: LDS atomicMax, so the
//      table never depends on thread order).  Longest match
//      wins, ties go to the smallest distance; lengths 3-258, distances 1-32 768, never before the block start; a
//      3-byte match farther than 4 096 back is dropped (zlib's TOO_FAR).
//   3. A lazy parse by wave 0 one chunk behind: the first position whose match the next position does not beat takes
//      its match, the positions before it are literals — 64 positions per step by ballot.  Tokens go to a scratch
//      slice of the block; the histograms are LDS counters.
//   4. Dynamic Huffman codes (RFC 1951 §3.2.2): lengths by the two-queue method over the sorted frequencies, limited to
//      15 bits (7 for the code-length alphabet) by moving leaves down/up until the Kraft sum is exactly 1; at least two
//      codes per tree (zlib's rule), HLIT/HDIST/HCLEN with the run codes 16/17/18 (svx_deflate_huff.h).
//   5. Bit lengths per token, a prefix sum per 256 tokens, ORs into LDS words.  A block whose DEFLATE form is not
//      smaller than a stored block (BTYPE 00) is written stored instead: every member is at most 65 536 bytes.
// A second kernel places the members one behind the other (their sizes scanned on the device) and appends the 28-byte
// EOF member.  Everything is a function of the block's bytes alone: the same input gives the same output however the
// blocks are split across launches.
#include <atomic>

#include "svx_deflate_huff.h"
#include "svx_internal.h"

namespace {

constexpr uint32_t kBlk = 65280u;      // input bytes per BGZF block (htslib BGZF_BLOCK_SIZE)
constexpr uint32_t kStride = 65536u;   // staging room per member (a stored member is 65 311 bytes)
constexpr int kThreads = 256;
constexpr int kHashBits = 12, kBuckets = 1 << kHashBits, kWays = 4;
constexpr uint32_t kSlotEmpty = 0xFFFFu;
constexpr uint32_t kTooFar = 4096u;
constexpr uint32_t kSliceBlocks = 2048u;  // blocks per launch (token scratch 255 KB each)

__constant__ uint16_t c_len_base[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31,
                                        35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
__constant__ uint8_t c_len_extra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
__constant__ uint16_t c_dist_base[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769,
                                         1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
__constant__ uint8_t c_dist_extra[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
__constant__ uint8_t c_cl_order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

struct DefArgs {
    const uint8_t* in;
    uint64_t n;            // bytes of the whole input
    uint32_t first;        // first block of this launch
    uint32_t count;        // blocks in this launch
    uint8_t* stage;        // count * kStride: member of block (first + i) at i * kStride
    uint32_t* tok;         // count * kBlk tokens
    uint32_t* mlen;        // member sizes, indexed by block
    uint32_t shift[6][32]; // x -> x * z^(8 * 1024 * 2^j) in CRC-32's field (svx_crc32_shift_columns)
};

struct Lds {
    uint32_t data[16386];                 // the block (zero-padded), then the packed DEFLATE bits
    union {
        struct {
            uint16_t slot[kBuckets][kWays];  // earlier positions per hash bucket, most recent first
            uint32_t latest[kBuckets];       // last position of the current chunk per bucket
        } t;
        struct {
            HuffWork lit, dist, cl;
        } h;
    } u;
    uint32_t mbuf[2][256];                // len << 16 | dist of the positions of a chunk (0: no match)
    uint16_t chash[256];                  // hash of every position of the chunk being matched (0xFFFF: none)
    uint32_t crc_tab[256];
    uint32_t lit_freq[288], dist_freq[32], cl_freq[20];
    uint8_t lit_len[288], dist_len[32], cl_len[20];
    uint16_t lit_code[288], dist_code[32], cl_code[20];
    uint16_t rle[320];                    // code-length symbols: sym | extra << 8
    uint32_t wsum[4];
    uint32_t hdr_bits, n_tok, n_rle, hlit, hdist, hclen;
    uint32_t tok_bits;
    uint32_t crc;
};

__device__ __forceinline__ uint8_t byte_at(const Lds& s, uint32_t i) {
    return reinterpret_cast<const uint8_t*>(s.data)[i];
}

__device__ __forceinline__ uint32_t hash3(const Lds& s, uint32_t q) {
    const uint32_t v = (uint32_t)byte_at(s, q) | (uint32_t)byte_at(s, q + 1) << 8 | (uint32_t)byte_at(s, q + 2) << 16;
    return (v * 2654435761u) >> (32 - kHashBits);
}

__device__ __forceinline__ uint32_t len_code(uint32_t len) {  // 257..285
    uint32_t c = 0;
    while (c < 28 && c_len_base[c + 1] <= len) ++c;
    return c;
}
__device__ __forceinline__ uint32_t dist_code(uint32_t d) {  // 0..29
    uint32_t lo = 0, hi = 29;
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1) >> 1;
        if (c_dist_base[mid] <= d) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ uint32_t crc_apply(const uint32_t (&col)[32], uint32_t x) {
    uint32_t r = 0;
#pragma unroll
    for (int i = 0; i < 32; ++i) r ^= (0u - ((x >> i) & 1u)) & col[i];
    return r;
}

// OR `nb` (<= 32) bits of v into the stream at bit `pos` (LDS words; atomic: neighbouring tokens share words)
__device__ __forceinline__ void put_bits(Lds& s, uint32_t pos, uint32_t v, uint32_t nb) {
    if (!nb) return;
    const uint64_t x = (uint64_t)(v & (nb == 32 ? 0xFFFFFFFFu : ((1u << nb) - 1u))) << (pos & 31u);
    atomicOr(&s.data[pos >> 5], (uint32_t)x);
    if ((uint32_t)(x >> 32)) atomicOr(&s.data[(pos >> 5) + 1], (uint32_t)(x >> 32));
}

__global__ __launch_bounds__(kThreads) void k_bgzf_deflate(DefArgs a) {
    extern __shared__ __align__(16) uint8_t lds_raw[];
    Lds& s = *reinterpret_cast<Lds*>(lds_raw);
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t blk = a.first + blockIdx.x;
    const uint64_t base = (uint64_t)blk * kBlk;
    const uint32_t n = (uint32_t)((a.n - base) < kBlk ? (a.n - base) : kBlk);  // 1..kBlk
    const uint8_t* src = a.in + base;
    uint32_t* tok = a.tok + (uint64_t)blockIdx.x * kBlk;
    uint8_t* dst = a.stage + (uint64_t)blockIdx.x * kStride;

    // ---- stage the block, clear the tables
    for (uint32_t i = tid; i < 16386u; i += kThreads) {
        uint32_t w = 0;
        const uint32_t b0 = i * 4u;
        for (uint32_t k = 0; k < 4; ++k)
            if (b0 + k < n) w |= (uint32_t)src[b0 + k] << (8 * k);
        s.data[i] = w;
    }
    for (uint32_t i = tid; i < (uint32_t)kBuckets; i += kThreads) {
        for (int k = 0; k < kWays; ++k) s.u.t.slot[i][k] = (uint16_t)kSlotEmpty;
        s.u.t.latest[i] = 0;
    }
    for (uint32_t i = tid; i < 288u; i += kThreads) s.lit_freq[i] = 0;
    if (tid < 32) s.dist_freq[tid] = 0;
    if (tid < 20) s.cl_freq[tid] = 0;
    {
        uint32_t c = tid;
        for (int k = 0; k < 8; ++k) c = (c & 1u) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
        s.crc_tab[tid] = c;
    }
    __syncthreads();

    // ---- CRC-32 (wave 0): pieces of 1 KiB, the last on lane 63, the odd-sized one first
    if (wave == 0) {
        const uint32_t n_pc = (n + 1023u) / 1024u;  // 1..64
        const uint32_t first_lane = 64u - n_pc, r = n - (n_pc - 1u) * 1024u;
        uint32_t state = 0;
        if (lane >= first_lane) {
            const uint32_t k = lane - first_lane;
            const uint32_t lo = k == 0 ? 0u : r + (k - 1u) * 1024u, hi = k == 0 ? r : lo + 1024u;
            uint32_t crc = k == 0 ? 0xFFFFFFFFu : 0u;
            for (uint32_t i = lo; i < hi; ++i) crc = s.crc_tab[(crc ^ byte_at(s, i)) & 0xFFu] ^ (crc >> 8);
            state = crc;
        }
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            uint32_t col[32];
#pragma unroll
            for (int i = 0; i < 32; ++i) col[i] = a.shift[j][i];
            const uint32_t right = (uint32_t)__shfl_down((int)state, 1 << j);
            const uint32_t folded = crc_apply(col, state) ^ right;
            if ((lane & ((2u << j) - 1u)) == 0) state = folded;
        }
        if (lane == 0) s.crc = state ^ 0xFFFFFFFFu;
    }

    // ---- LZ77: chunk c matched by all threads; wave 0 parses chunk c - 1 behind it
    const uint32_t n_chunks = (n + 255u) / 256u;
    uint32_t p = 0, ntok = 0;  // the parse (wave 0, uniform)
    auto parse_chunk = [&](uint32_t c) {
        const uint32_t end = (c + 1u) * 256u < n ? (c + 1u) * 256u : n;
        while (p < end) {
            const uint32_t q = p + lane;
            const bool valid = q < end;
            const uint32_t m = valid ? s.mbuf[(q >> 8) & 1u][q & 255u] : 0u;
            const uint32_t ln = m >> 16;
            uint32_t nx = 0;
            if (valid && q + 1u < n && ln >= 3u) nx = s.mbuf[((q + 1u) >> 8) & 1u][(q + 1u) & 255u] >> 16;
            const bool cand = valid && ln >= 3u && nx <= ln;
            const uint64_t ball = __ballot(cand);
            const uint32_t avail = end - p < 64u ? end - p : 64u;
            const uint32_t f = ball ? (uint32_t)__builtin_ctzll(ball) : avail;  // literals in front of the match
            if (lane < f) {
                const uint32_t b = byte_at(s, q);
                tok[ntok + lane] = b;
                atomicAdd(&s.lit_freq[b], 1u);
            }
            const uint32_t mm = (uint32_t)__shfl((int)m, (int)(f & 63u));
            if (ball) {
                const uint32_t L = mm >> 16, D = mm & 0xFFFFu;
                if (lane == f) {
                    tok[ntok + f] = 0x80000000u | (L - 3u) << 16 | (D - 1u);
                    atomicAdd(&s.lit_freq[257u + len_code(L)], 1u);
                    atomicAdd(&s.dist_freq[dist_code(D)], 1u);
                }
                p += f + L;
                ntok += f + 1u;
            } else {
                p += f;
                ntok += f;
            }
        }
    };
    for (uint32_t c = 0; c <= n_chunks; ++c) {
        const uint32_t q = c * 256u + tid;
        uint32_t h = 0;
        const bool hashed = c < n_chunks && q + 3u <= n;
        if (hashed) h = hash3(s, q);
        s.chash[tid] = hashed ? (uint16_t)h : (uint16_t)0xFFFFu;
        __syncthreads();
        if (c < n_chunks) {
            uint32_t best = 0, bd = 0;
            if (hashed) {
                const uint32_t maxlen = n - q < 258u ? n - q : 258u;
                auto try_at = [&](uint32_t from) {
                    const uint32_t d = q - from;
                    if (d == 0 || d > 32768u) return;
                    uint32_t l = 0;
                    while (l < maxlen && byte_at(s, from + l) == byte_at(s, q + l)) ++l;
                    if (l == 3u && d > kTooFar) l = 0;
                    if (l >= 3u && (l > best || (l == best && d < bd))) { best = l; bd = d; }
                };
                for (uint32_t d = 1; d <= 4u && d <= q; ++d) try_at(q - d);
                // the nearest earlier positions of the same hash inside this chunk (the table holds earlier chunks only)
                uint32_t found = 0;
                for (int j = (int)tid - 5; j >= 0 && found < 4u; --j)
                    if (s.chash[j] == h) {
                        try_at(c * 256u + (uint32_t)j);
                        ++found;
                    }
                for (int k = 0; k < kWays; ++k) {
                    const uint32_t at = s.u.t.slot[h][k];
                    if (at != kSlotEmpty) try_at(at);
                }
            }
            s.mbuf[c & 1u][tid] = best >= 3u ? (best << 16 | bd) : 0u;
        }
        __syncthreads();
        if (hashed) atomicMax(&s.u.t.latest[h], q);
        if (wave == 0 && c > 0) parse_chunk(c - 1u);
        __syncthreads();
        if (hashed && s.u.t.latest[h] == q) {
            for (int k = kWays - 1; k > 0; --k) s.u.t.slot[h][k] = s.u.t.slot[h][k - 1];
            s.u.t.slot[h][0] = (uint16_t)q;
        }
        __syncthreads();
    }
    if (tid == 0) {
        s.n_tok = ntok;
        s.lit_freq[256] = 1;  // end of block
    }
    __syncthreads();

    // ---- Huffman code lengths: literal/length on wave 0, distance on wave 1; the block's bytes are dead: clear them
    for (uint32_t i = tid; i < 16386u; i += kThreads) s.data[i] = 0;
    if (tid == 0) build_lengths(s.lit_freq, 286, 15, s.lit_len, s.u.h.lit);
    if (tid == 64) build_lengths(s.dist_freq, 30, 15, s.dist_len, s.u.h.dist);
    if (tid == 0) { s.lit_len[286] = 0; s.lit_len[287] = 0; }
    __syncthreads();
    if (tid == 0) {
        uint32_t hlit = 286, hdist = 30;
        while (hlit > 257 && s.lit_len[hlit - 1] == 0) --hlit;
        while (hdist > 1 && s.dist_len[hdist - 1] == 0) --hdist;
        const uint32_t nr = rle_lengths(s.lit_len, hlit, s.dist_len, hdist, s.rle);
        for (uint32_t k = 0; k < nr; ++k) s.cl_freq[s.rle[k] & 0xFFu]++;
        build_lengths(s.cl_freq, 19, 7, s.cl_len, s.u.h.cl);
        uint32_t hclen = 19;
        while (hclen > 4 && s.cl_len[c_cl_order[hclen - 1]] == 0) --hclen;
        make_codes(s.lit_len, 286, s.lit_code);
        make_codes(s.dist_len, 30, s.dist_code);
        make_codes(s.cl_len, 19, s.cl_code);
        // the header: BFINAL 1, BTYPE 10
        uint32_t pos = 0;
        put_bits(s, pos, 1u | 2u << 1, 3); pos += 3;
        put_bits(s, pos, hlit - 257u, 5); pos += 5;
        put_bits(s, pos, hdist - 1u, 5); pos += 5;
        put_bits(s, pos, hclen - 4u, 4); pos += 4;
        for (uint32_t k = 0; k < hclen; ++k) { put_bits(s, pos, s.cl_len[c_cl_order[k]], 3); pos += 3; }
        for (uint32_t k = 0; k < nr; ++k) {
            const uint32_t sym = s.rle[k] & 0xFFu, ex = s.rle[k] >> 8;
            put_bits(s, pos, s.cl_code[sym], s.cl_len[sym]); pos += s.cl_len[sym];
            const uint32_t eb = sym == 16 ? 2u : sym == 17 ? 3u : sym == 18 ? 7u : 0u;
            put_bits(s, pos, ex, eb); pos += eb;
        }
        s.hdr_bits = pos;
        s.tok_bits = 0;
    }
    __syncthreads();

    // ---- the tokens' bits: total first (stored or not), then the packing
    const uint32_t nt = s.n_tok;
    auto tok_bits = [&](uint32_t t, uint32_t& v1, uint32_t& b1, uint32_t& v2, uint32_t& b2) {
        const uint32_t x = tok[t];
        if (!(x & 0x80000000u)) {
            v1 = s.lit_code[x]; b1 = s.lit_len[x]; v2 = 0; b2 = 0;
            return;
        }
        const uint32_t L = ((x >> 16) & 0xFFu) + 3u, D = (x & 0xFFFFu) + 1u;
        const uint32_t lc = len_code(L), dc = dist_code(D);
        const uint32_t ls = 257u + lc;
        v1 = s.lit_code[ls] | (L - c_len_base[lc]) << s.lit_len[ls];
        b1 = s.lit_len[ls] + c_len_extra[lc];
        v2 = s.dist_code[dc] | (D - c_dist_base[dc]) << s.dist_len[dc];
        b2 = s.dist_len[dc] + c_dist_extra[dc];
    };
    uint32_t mine = 0;
    for (uint32_t t = tid; t < nt; t += kThreads) {
        uint32_t v1, b1, v2, b2;
        tok_bits(t, v1, b1, v2, b2);
        mine += b1 + b2;
    }
    atomicAdd(&s.tok_bits, mine);
    __syncthreads();
    const uint32_t bits = s.hdr_bits + s.tok_bits + s.lit_len[256];
    const uint32_t zbytes = (bits + 7u) / 8u;
    const bool stored = zbytes >= n + 5u;
    const uint32_t crc = s.crc;
    if (!stored) {
        uint32_t at = s.hdr_bits;  // uniform
        for (uint32_t t0 = 0; t0 < nt; t0 += kThreads) {
            const uint32_t t = t0 + tid;
            uint32_t v1 = 0, b1 = 0, v2 = 0, b2 = 0;
            if (t < nt) tok_bits(t, v1, b1, v2, b2);
            // block-wide exclusive scan of b1 + b2
            uint32_t x = b1 + b2, incl = x;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t y = (uint32_t)__shfl_up((int)incl, o);
                if (lane >= (uint32_t)o) incl += y;
            }
            if (lane == 63) s.wsum[wave] = incl;
            __syncthreads();
            uint32_t before = 0, all = 0;
            for (uint32_t w = 0; w < 4; ++w) {
                if (w < wave) before += s.wsum[w];
                all += s.wsum[w];
            }
            const uint32_t pos = at + before + incl - x;
            put_bits(s, pos, v1, b1);
            put_bits(s, pos + b1, v2, b2);
            at += all;
            __syncthreads();
        }
        if (tid == 0) put_bits(s, at, s.lit_code[256], s.lit_len[256]);
        __syncthreads();
    }
    // ---- the member: header, DEFLATE data, CRC32, ISIZE
    const uint32_t body = stored ? n + 5u : zbytes;
    const uint32_t msize = 18u + body + 8u;
    if (tid < 18) {
        const uint8_t hdr[18] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0,
                                 (uint8_t)((msize - 1u) & 0xFFu), (uint8_t)((msize - 1u) >> 8)};
        dst[tid] = hdr[tid];
    } else if (tid < 26) {
        const uint32_t k = tid - 18u;
        dst[18u + body + k] = (uint8_t)((k < 4 ? crc : n) >> (8 * (k & 3u)));
    }
    if (stored) {
        if (tid < 5) {
            const uint8_t sh[5] = {1, (uint8_t)(n & 0xFFu), (uint8_t)(n >> 8), (uint8_t)(~n & 0xFFu), (uint8_t)((~n >> 8) & 0xFFu)};
            dst[18u + tid] = sh[tid];
        }
        for (uint32_t i = tid; i < n; i += kThreads) dst[23u + i] = src[i];
    } else {
        const uint8_t* bytes = reinterpret_cast<const uint8_t*>(s.data);
        for (uint32_t i = tid; i < zbytes; i += kThreads) dst[18u + i] = bytes[i];
    }
    if (tid == 0) a.mlen[blk] = msize;
}

// offsets of the members (exclusive scan of the sizes, one workgroup), the total with the EOF member behind
__global__ __launch_bounds__(kThreads) void k_member_offsets(const uint32_t* __restrict__ mlen, uint32_t n_blk,
                                                             uint64_t* __restrict__ off, uint64_t* __restrict__ total) {
    __shared__ uint64_t wsum[4];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint64_t run = 0;
    for (uint32_t b0 = 0; b0 < n_blk; b0 += kThreads) {
        const uint32_t b = b0 + tid;
        const uint64_t x = b < n_blk ? mlen[b] : 0u;
        uint64_t incl = x;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint64_t y = __shfl_up(incl, o);
            if (lane >= (uint32_t)o) incl += y;
        }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        uint64_t before = 0, all = 0;
        for (uint32_t w = 0; w < 4; ++w) {
            if (w < wave) before += wsum[w];
            all += wsum[w];
        }
        if (b < n_blk) off[b] = run + before + incl - x;
        run += all;
        __syncthreads();
    }
    if (tid == 0) {
        off[n_blk] = run;
        *total = run + 28u;
    }
}

// the staged members of one launch to their places in the output; the last workgroup of the last launch adds the EOF
__global__ __launch_bounds__(kThreads) void k_member_gather(const uint8_t* __restrict__ stage, const uint32_t* __restrict__ mlen,
                                                            const uint64_t* __restrict__ off, uint32_t first, uint32_t count,
                                                            uint32_t n_blk, uint8_t* __restrict__ out) {
    if (blockIdx.x == count) {
        if (first + count != n_blk) return;
        const uint8_t eof[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        if (threadIdx.x < 28) out[off[n_blk] + threadIdx.x] = eof[threadIdx.x];
        return;
    }
    const uint32_t b = first + blockIdx.x;
    const uint8_t* s = stage + (uint64_t)blockIdx.x * kStride;
    uint8_t* d = out + off[b];
    const uint32_t l = mlen[b];
    for (uint32_t i = threadIdx.x; i < l; i += kThreads) d[i] = s[i];
}

}  // namespace

extern "C" uint64_t svx_bgzf_deflate_bound(uint64_t n) {
    return (n + kBlk - 1u) / kBlk * (uint64_t)kStride + 28u;
}

// on a stream of the caller's, scratch from the caller: hipError_t as int, or -1 for bad arguments
static int deflate_on_stream(hipStream_t stream, const uint8_t* d_in, uint64_t n, uint8_t* d_out, uint32_t* d_mlen,
                             uint64_t* d_off, uint64_t* d_total, uint8_t* d_stage, uint32_t* d_tok, uint32_t slice) {
    const uint64_t n_blk64 = (n + kBlk - 1u) / kBlk;
    const uint32_t n_blk = (uint32_t)n_blk64;
    const hipError_t lds_set = hipFuncSetAttribute(reinterpret_cast<const void*>(k_bgzf_deflate),
                                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(Lds));
    if (lds_set != hipSuccess) return (int)lds_set;
    DefArgs a;
    a.in = d_in;
    a.n = n;
    a.stage = d_stage;
    a.tok = d_tok;
    a.mlen = d_mlen;
    memcpy(a.shift, svx_crc32_shift_columns(), sizeof(a.shift));
    // one slice: compress into the stage, scan the sizes, gather the members into place behind each other
    if (n_blk <= slice) {
        a.first = 0;
        a.count = n_blk;
        if (n_blk) hipLaunchKernelGGL(k_bgzf_deflate, dim3(n_blk), dim3(kThreads), sizeof(Lds), stream, a);
        hipLaunchKernelGGL(k_member_offsets, dim3(1), dim3(kThreads), 0, stream, d_mlen, n_blk, d_off, d_total);
        hipLaunchKernelGGL(k_member_gather, dim3(n_blk + 1), dim3(kThreads), 0, stream, d_stage, d_mlen, d_off, 0u, n_blk, n_blk, d_out);
        return (int)hipGetLastError();
    }
    // many slices: compress each slice into the stage and place it at a fixed stride in the output (the bound leaves
    // room for that), then scan the sizes and move the members down into place in order — members only move towards
    // the front, and block b lands at or before b * kStride, which block b no longer needs after its own copy
    for (uint32_t first = 0; first < n_blk; first += slice) {
        a.first = first;
        a.count = n_blk - first < slice ? n_blk - first : slice;
        hipLaunchKernelGGL(k_bgzf_deflate, dim3(a.count), dim3(kThreads), sizeof(Lds), stream, a);
        hipError_t e = hipMemcpyAsync(d_out + (uint64_t)first * kStride, d_stage, (uint64_t)a.count * kStride, hipMemcpyDeviceToDevice, stream);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(k_member_offsets, dim3(1), dim3(kThreads), 0, stream, d_mlen, n_blk, d_off, d_total);
    // slice by slice through the stage: the slices in front have written nothing beyond (first * kStride), since
    // off[b] + mlen[b] <= (b + 1) * kStride for every member (each is below kStride bytes)
    for (uint32_t first = 0; first < n_blk; first += slice) {
        const uint32_t count = n_blk - first < slice ? n_blk - first : slice;
        hipError_t e = hipMemcpyAsync(d_stage, d_out + (uint64_t)first * kStride, (uint64_t)count * kStride, hipMemcpyDeviceToDevice, stream);
        if (e != hipSuccess) return (int)e;
        hipLaunchKernelGGL(k_member_gather, dim3(count + 1), dim3(kThreads), 0, stream, d_stage, d_mlen, d_off, first, count, n_blk, d_out);
    }
    return (int)hipGetLastError();
}

static std::atomic<uint32_t> g_slice{kSliceBlocks};
extern "C" uint32_t svx_bgzf_deflate_set_slice(uint32_t blocks) {
    return g_slice.exchange(blocks ? blocks : kSliceBlocks);
}

extern "C" int svx_bgzf_deflate_dev(svx_ctx* ctx, const uint8_t* d_in, uint64_t n, uint8_t* d_out, uint64_t cap,
                                    uint32_t* d_member_len, uint64_t* d_total) {
    if (!ctx || !d_out || !d_total || (n && (!d_in || !d_member_len))) return SVX_E_INVALID;
    if (cap < svx_bgzf_deflate_bound(n)) {
        SVX_SET_ERR(ctx, "svx_bgzf_deflate_dev: cap %llu < bound %llu", (unsigned long long)cap,
                    (unsigned long long)svx_bgzf_deflate_bound(n));
        return SVX_E_CAPACITY;
    }
    const uint64_t n_blk = (n + kBlk - 1u) / kBlk;
    if (n_blk >= 0xFFFFFFFFull) return SVX_E_TOO_LARGE;
    SVX_HIP(ctx, hipSetDevice(ctx->device));
    const uint32_t slice = g_slice.load();
    const uint64_t per = n_blk < slice ? n_blk : slice;
    uint64_t* d_off;
    uint8_t* d_stage;
    uint32_t* d_tok;
    svx_takes ws;
    ws.add(&d_off, n_blk + 1);
    ws.add(&d_stage, per * kStride);
    ws.add(&d_tok, per * kBlk);
    SVX_TRY(svx_ws_lay(ctx, ws));
    SVX_TRY(svx_timing_begin(ctx));
    SVX_TRY(svx_timing_mark(ctx, 1));
    SVX_HIP(ctx, (hipError_t)deflate_on_stream(ctx->stream, d_in, n, d_out, d_member_len, d_off, d_total, d_stage, d_tok, slice));
    SVX_TRY(svx_timing_mark(ctx, 2));
    return svx_timing_end(ctx);
}

// ------------------------------------------------------------------------------------------------ host bytes
#include <zlib.h>

#include <thread>
#include <vector>

namespace {

constexpr uint8_t kEof[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};

// one block as bgzip writes it with zlib (raw deflate, level 6), or stored where that is not smaller; returns the size
uint32_t zlib_member(const uint8_t* src, uint32_t n, uint8_t* dst, bool& ok) {
    z_stream z;
    memset(&z, 0, sizeof(z));
    uint32_t body = 0;
    if (deflateInit2(&z, 6, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) != Z_OK) {
        ok = false;
        return 0;
    }
    z.next_in = const_cast<uint8_t*>(src);
    z.avail_in = n;
    z.next_out = dst + 18;
    z.avail_out = n + 4;  // less than a stored block, or it is stored
    const int rc = deflate(&z, Z_FINISH);
    const bool fits = rc == Z_STREAM_END && z.total_out < (uLong)n + 5u;
    body = fits ? (uint32_t)z.total_out : 0u;
    deflateEnd(&z);
    if (!fits) {
        dst[18] = 1;
        dst[19] = (uint8_t)n;
        dst[20] = (uint8_t)(n >> 8);
        dst[21] = (uint8_t)~n;
        dst[22] = (uint8_t)(~n >> 8);
        memcpy(dst + 23, src, n);
        body = n + 5u;
    }
    const uint32_t msize = 18u + body + 8u;
    const uint8_t hdr[18] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0,
                             (uint8_t)((msize - 1u) & 0xFFu), (uint8_t)((msize - 1u) >> 8)};
    memcpy(dst, hdr, 18);
    const uint32_t crc = (uint32_t)crc32(crc32(0L, Z_NULL, 0), src, n);
    for (int k = 0; k < 4; ++k) {
        dst[18 + body + k] = (uint8_t)(crc >> (8 * k));
        dst[22 + body + k] = (uint8_t)(n >> (8 * k));
    }
    return msize;
}

int compress_host(const uint8_t* src, uint64_t n, int n_threads, uint8_t** out, uint64_t* out_len, uint32_t** mlen, uint64_t* n_members) {
    const uint64_t n_blk = (n + kBlk - 1u) / kBlk;
    std::vector<uint8_t> stage;
    uint32_t* sizes = (uint32_t*)malloc(n_blk ? n_blk * 4 : 4);
    if (!sizes) return SVX_E_NOMEM;
    try {
        stage.resize(n_blk * kStride);
    } catch (const std::bad_alloc&) {
        free(sizes);
        return SVX_E_NOMEM;
    }
    unsigned nt = n_threads > 0 ? (unsigned)n_threads : std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    if ((uint64_t)nt > n_blk) nt = n_blk ? (unsigned)n_blk : 1u;
    std::atomic<uint64_t> next{0};
    std::atomic<bool> ok{true};
    auto work = [&] {
        for (uint64_t b; (b = next.fetch_add(1)) < n_blk;) {
            const uint64_t at = b * kBlk;
            const uint32_t len = (uint32_t)(n - at < kBlk ? n - at : kBlk);
            bool fine = true;
            sizes[b] = zlib_member(src + at, len, stage.data() + b * kStride, fine);
            if (!fine) ok = false;
        }
    };
    if (nt <= 1) {
        work();
    } else {
        std::vector<std::thread> th;
        for (unsigned t = 0; t < nt; ++t) th.emplace_back(work);
        for (std::thread& t : th) t.join();
    }
    if (!ok) {
        free(sizes);
        return SVX_E_NOMEM;
    }
    uint64_t total = 28;
    for (uint64_t b = 0; b < n_blk; ++b) total += sizes[b];
    uint8_t* buf = (uint8_t*)malloc(total);
    if (!buf) {
        free(sizes);
        return SVX_E_NOMEM;
    }
    uint64_t at = 0;
    for (uint64_t b = 0; b < n_blk; ++b) {
        memcpy(buf + at, stage.data() + b * kStride, sizes[b]);
        at += sizes[b];
    }
    memcpy(buf + at, kEof, 28);
    *out = buf;
    *out_len = total;
    *mlen = sizes;
    *n_members = n_blk;
    return SVX_OK;
}

int compress_device(svx_ctx* ctx, const uint8_t* src, uint64_t n, uint8_t** out, uint64_t* out_len, uint32_t** mlen, uint64_t* n_members) {
    const uint64_t n_blk = (n + kBlk - 1u) / kBlk;
    const uint64_t bound = svx_bgzf_deflate_bound(n);
    SVX_HIP(ctx, hipSetDevice(ctx->device));
    uint8_t *d_in, *d_out;
    uint32_t* d_mlen;
    uint64_t* d_total;
    svx_takes st;
    if (n) st.add_up(&d_in, src, n); else st.add(&d_in, 1);
    st.add(&d_out, bound);
    st.add(&d_mlen, n_blk + 1);
    st.add(&d_total, 1);
    SVX_TRY(svx_stage_lay(ctx, st));
    SVX_TRY(svx_bgzf_deflate_dev(ctx, d_in, n, d_out, bound, d_mlen, d_total));
    uint32_t* sizes = (uint32_t*)malloc(n_blk ? n_blk * 4 : 4);
    if (!sizes) return SVX_E_NOMEM;
    uint64_t total = 0;
    hipError_t e = hipMemcpyAsync(&total, d_total, 8, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && n_blk) e = hipMemcpyAsync(sizes, d_mlen, n_blk * 4, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    uint8_t* buf = nullptr;
    if (e == hipSuccess && total <= bound) {
        buf = (uint8_t*)malloc(total);
        if (!buf) {
            free(sizes);
            return SVX_E_NOMEM;
        }
        e = hipMemcpyAsync(buf, d_out, total, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    }
    if (e != hipSuccess || total > bound) {
        free(sizes);
        free(buf);
        SVX_SET_ERR(ctx, "svx_bgzf_compress: %s", e != hipSuccess ? hipGetErrorString(e) : "output beyond its bound");
        return e == hipErrorOutOfMemory ? SVX_E_NOMEM : SVX_E_HIP;
    }
    *out = buf;
    *out_len = total;
    *mlen = sizes;
    *n_members = n_blk;
    return SVX_OK;
}

}  // namespace

extern "C" int svx_bgzf_compress(svx_ctx* ctx, const uint8_t* src, uint64_t n, int n_threads, uint8_t** out, uint64_t* out_len,
                                 uint32_t** member_len, uint64_t* n_members) {
    if (!out || !out_len || !member_len || !n_members || (n && !src)) return SVX_E_INVALID;
    *out = nullptr;
    *member_len = nullptr;
    *out_len = 0;
    *n_members = 0;
    try {
        return ctx ? compress_device(ctx, src, n, out, out_len, member_len, n_members)
                   : compress_host(src, n, n_threads, out, out_len, member_len, n_members);
    } catch (const std::bad_alloc&) {
        return SVX_E_NOMEM;
    } catch (...) {
        return SVX_E_INVALID;
    }
}

extern "C" void svx_bgzf_free(void* p) { free(p); }
