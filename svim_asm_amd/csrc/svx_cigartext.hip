// svx_cigartext.hip — CIGAR text ("12M3I40M…") of many records → BAM words (`len << 4 | op`) on the device:
// svx_cigar_text_parse_dev (include/svx_sam.h), and the launch the SAM reader (svx_sam.cpp) takes through a pointer.
//
// The input is the CIGAR fields of the records back to back, text[n_bytes], and rec_off[n_rec + 1]; positions are global,
// so a number or a record may lie across any chunk boundary.  A byte that is neither a digit nor '*' is an OPERATOR BYTE;
// a record without an error yields one word per operator byte, in text order.
//
//   k_count    a workgroup per chunk of kChunk bytes, a byte per lane and step: classifies the bytes, counts the chunk's
//              operator bytes (ballot + popcount, summed over the waves through LDS) and judges every operator byte —
//              character, operator letter, the number in front of it (read backwards from the byte, across chunk
//              boundaries, down to the record's start) — noting the EARLIEST error of a record as min(position << 3 | code)
//   k_scan     exclusive sum of the chunk counts: the rank of every chunk's first operator byte among all of them
//   k_rec_rank a wave per record boundary: the rank of the first operator byte at or behind rec_off[r]
//   k_rec_fin  a lane per record: empty text, a digit as the last byte; status; the
//              record's operator count (0 for a record with an error) — then k_scan again gives cigar_off
//   k_emit     k_count's walk again: an operator byte's word index is cigar_off[r] + (its rank - the rank at the record's
//              start), its rank inside the chunk from mbcnt over the ballot mask; ref_len is a segmented sum: a wave that
//              lies inside one record adds its lanes up first and sends one atomic, the others one per lane
// All stores are vector stores; the only atomics are the vector ones on the per-record error keys and ref_len.
#include <hip/hip_runtime.h>

#include "svx_internal.h"
#include "svx_cigartext_dev.h"
#include "svx_sam.h"

namespace {

constexpr int kThreads = 256;
constexpr uint32_t kChunk = 1024;  // bytes per workgroup: four steps of a byte per lane
constexpr int kWaves = kThreads / 64;

__device__ __forceinline__ bool is_digit(uint32_t c) { return c - '0' < 10u; }
__device__ __forceinline__ bool is_opbyte(uint32_t c) { return !is_digit(c) && c != '*'; }

// M I D N S H P = X -> 0..8; 15: a letter that is no operator; 14: no letter at all
__device__ __forceinline__ uint32_t op_code(uint32_t c) {
    switch (c) {
        case 'M': return 0; case 'I': return 1; case 'D': return 2; case 'N': return 3; case 'S': return 4;
        case 'H': return 5; case 'P': return 6; case '=': return 7; case 'X': return 8;
        default: break;
    }
    return ((c | 32u) - 'a' < 26u) ? 15u : 14u;
}

// last r with rec_off[r] <= p (records of no bytes share an offset with the one that holds p: the last of them holds it)
__device__ __forceinline__ uint32_t record_of(const uint64_t* __restrict__ rec_off, uint32_t n_rec, uint64_t p) {
    uint32_t lo = 0, hi = n_rec;  // rec_off[lo] <= p < rec_off[hi]
    while (hi - lo > 1) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (rec_off[mid] <= p) lo = mid; else hi = mid;
    }
    return lo;
}

// the number that ends in front of byte p, read backwards down to `start`: digits, value (exact below 10^10, `big` set when it
// is at least 2^28)
__device__ __forceinline__ uint32_t number_before(const uint8_t* __restrict__ text, uint64_t start, uint64_t p, uint32_t* n_digits,
                                                  bool* big) {
    uint64_t v = 0, pw = 1;
    uint32_t k = 0;
    bool over = false;
    while (p > start) {
        const uint32_t c = text[p - 1];
        if (!is_digit(c)) break;
        if (k < 10) { v += (c - '0') * pw; pw *= 10; }
        else if (c != '0') over = true;
        --p;
        ++k;
    }
    *n_digits = k;
    *big = over || v >= (1ull << 28);
    return (uint32_t)v;
}

__device__ __forceinline__ uint32_t wave_rank(uint64_t mask) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

__global__ void __launch_bounds__(kThreads) k_count(const uint8_t* __restrict__ text, uint64_t n_bytes, const uint64_t* __restrict__ rec_off,
                                                   uint32_t n_rec, uint32_t* __restrict__ chunk_cnt,
                                                   unsigned long long* __restrict__ err_key) {
    __shared__ uint32_t s_cnt[kWaves];
    const uint64_t base = (uint64_t)blockIdx.x * kChunk;
    uint32_t mine = 0;
    for (uint32_t step = 0; step < kChunk / kThreads; ++step) {
        const uint64_t p = base + step * kThreads + threadIdx.x;
        const uint32_t c = p < n_bytes ? text[p] : (uint32_t)'0';
        const bool opb = is_opbyte(c);
        mine += (uint32_t)__popcll(__ballot(opb));  // (the same in every lane of the wave)
        if (c == '*') {  // the whole text of a record without a CIGAR, a bad character anywhere else
            const uint32_t r = record_of(rec_off, n_rec, p);
            if (rec_off[r + 1] - rec_off[r] != 1) atomicMin(&err_key[r], (unsigned long long)((p << 3) | SVX_CIGAR_BAD_CHAR));
        }
        if (opb) {
            const uint32_t r = record_of(rec_off, n_rec, p);
            const uint32_t code = op_code(c);
            uint32_t nd;
            bool big;
            (void)number_before(text, rec_off[r], p, &nd, &big);
            const uint32_t e = code == 14 ? SVX_CIGAR_BAD_CHAR : code == 15 ? SVX_CIGAR_BAD_OP : nd == 0 ? SVX_CIGAR_EMPTY_NUMBER
                               : big ? SVX_CIGAR_NUMBER_TOO_BIG : 0u;
            if (e) atomicMin(&err_key[r], (unsigned long long)((p << 3) | e));
        }
    }
    if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (int w = 0; w < kWaves; ++w) t += s_cnt[w];
        chunk_cnt[blockIdx.x] = t;
    }
}

// out[0..n] = exclusive sum of in[0..n): one workgroup, tiles of its size with a carry
constexpr int kScanThreads = 1024;
__global__ void __launch_bounds__(kScanThreads) k_scan(const uint32_t* __restrict__ in, uint64_t n, uint64_t* __restrict__ out) {
    __shared__ uint64_t s_wave[kScanThreads / 64];
    __shared__ uint64_t s_carry;
    if (threadIdx.x == 0) s_carry = 0;
    __syncthreads();
    for (uint64_t t0 = 0; t0 < n; t0 += kScanThreads) {
        const uint64_t i = t0 + threadIdx.x;
        const uint64_t v = i < n ? in[i] : 0;
        uint64_t x = v;  // inclusive sum inside the wave
        for (int d = 1; d < 64; d <<= 1) {
            const uint64_t y = __shfl_up(x, d);
            if ((int)(threadIdx.x & 63) >= d) x += y;
        }
        if ((threadIdx.x & 63) == 63) s_wave[threadIdx.x >> 6] = x;
        __syncthreads();
        uint64_t before = s_carry;
        for (uint32_t w = 0; w < (threadIdx.x >> 6); ++w) before += s_wave[w];
        if (i < n) out[i] = before + x - v;
        __syncthreads();
        if (threadIdx.x == kScanThreads - 1) s_carry = before + x;
        __syncthreads();
    }
    if (threadIdx.x == 0) out[n] = s_carry;
}

// rank[r] = operator bytes in text[0, rec_off[r]), r = 0..n_rec: the chunk's rank + the bytes of the chunk in front of it
__global__ void __launch_bounds__(kThreads) k_rec_rank(const uint8_t* __restrict__ text, uint64_t n_bytes, const uint64_t* __restrict__ rec_off,
                                                      uint32_t n_rec, const uint64_t* __restrict__ chunk_base, uint64_t* __restrict__ rank) {
    const uint32_t r = blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (r > n_rec) return;
    const uint64_t end = rec_off[r];
    const uint64_t ch = end / kChunk;
    uint32_t cnt = 0;
    for (uint64_t p = ch * kChunk + (threadIdx.x & 63); p - (threadIdx.x & 63) < end; p += 64)
        cnt += (uint32_t)__popcll(__ballot(p < end && is_opbyte(text[p])));
    if ((threadIdx.x & 63) == 0) rank[r] = chunk_base[ch] + cnt;  // (ch may be the chunk count: the sum's last entry)
}

__global__ void __launch_bounds__(kThreads) k_rec_fin(const uint8_t* __restrict__ text, const uint64_t* __restrict__ rec_off, uint32_t n_rec,
                                                     const uint64_t* __restrict__ rank, const unsigned long long* __restrict__ err_key,
                                                     uint32_t* __restrict__ status, uint32_t* __restrict__ n_ops) {
    const uint32_t r = blockIdx.x * kThreads + threadIdx.x;
    if (r >= n_rec) return;
    const uint64_t a = rec_off[r], b = rec_off[r + 1];
    unsigned long long key = err_key[r];
    if (b == a) {
        key = SVX_CIGAR_EMPTY_NUMBER;
    } else if (is_digit(text[b - 1])) {
        const unsigned long long k = ((b - 1) << 3) | SVX_CIGAR_TRAILING_DIGITS;
        if (k < key) key = k;
    }
    const uint32_t st = key == ~0ull ? 0u : (uint32_t)(key & 7);
    status[r] = st;
    n_ops[r] = st ? 0u : (uint32_t)(rank[r + 1] - rank[r]);
}

__global__ void __launch_bounds__(kThreads) k_emit(const uint8_t* __restrict__ text, uint64_t n_bytes, const uint64_t* __restrict__ rec_off,
                                                  uint32_t n_rec, const uint64_t* __restrict__ chunk_base, const uint64_t* __restrict__ rank,
                                                  const uint32_t* __restrict__ status, const uint64_t* __restrict__ cigar_off,
                                                  uint64_t cap, uint32_t* __restrict__ words, int32_t* __restrict__ ref_len) {
    __shared__ uint32_t s_cnt[kChunk / 64];
    const uint64_t base = (uint64_t)blockIdx.x * kChunk;
    const uint32_t wave = threadIdx.x >> 6;
    uint64_t masks[kChunk / kThreads];
    uint8_t cs[kChunk / kThreads];
#pragma unroll
    for (uint32_t step = 0; step < kChunk / kThreads; ++step) {
        const uint64_t p = base + step * kThreads + threadIdx.x;
        const uint32_t c = p < n_bytes ? text[p] : (uint32_t)'0';
        cs[step] = (uint8_t)c;
        masks[step] = __ballot(is_opbyte(c));
        if ((threadIdx.x & 63) == 0) s_cnt[step * kWaves + wave] = (uint32_t)__popcll(masks[step]);
    }
    __syncthreads();
    const uint64_t chunk_rank = chunk_base[blockIdx.x];
#pragma unroll
    for (uint32_t step = 0; step < kChunk / kThreads; ++step) {
        const uint64_t p0 = base + step * kThreads + wave * 64;  // the wave's first byte
        if (p0 >= n_bytes) break;
        uint32_t before = 0;
        for (uint32_t w = 0; w < step * kWaves + wave; ++w) before += s_cnt[w];
        const uint64_t p = p0 + (threadIdx.x & 63);
        const uint32_t c = cs[step];
        const bool opb = p < n_bytes && is_opbyte(c);
        const uint64_t p_last = p0 + 63 < n_bytes ? p0 + 63 : n_bytes - 1;
        const uint32_t r_first = record_of(rec_off, n_rec, p0), r_last = record_of(rec_off, n_rec, p_last);
        const bool one_record = r_first == r_last;
        uint32_t add = 0, r = r_first;
        if (opb) {
            if (!one_record) r = record_of(rec_off, n_rec, p);
            if (status[r] == 0) {
                uint32_t nd;
                bool big;
                const uint32_t v = number_before(text, rec_off[r], p, &nd, &big);
                const uint32_t code = op_code(c);
                const uint64_t idx = cigar_off[r] + (chunk_rank + before + wave_rank(masks[step]) - rank[r]);
                if (idx < cap) words[idx] = (v << 4) | code;
                if ((0x18Du >> code) & 1u) add = v;  // M D N = X consume the reference
            }
        }
        if (one_record) {
            for (int d = 32; d > 0; d >>= 1) add += __shfl_xor(add, d);
            if ((threadIdx.x & 63) == 0 && add) atomicAdd(reinterpret_cast<uint32_t*>(&ref_len[r_first]), add);
        } else if (add) {
            atomicAdd(reinterpret_cast<uint32_t*>(&ref_len[r]), add);
        }
    }
}

}  // namespace

// the parser's scratch: what the need-function measures, the SAM reader's launcher places in its own buffer and the context's
// entry lays out in the workspace
struct TextScratch {
    uint64_t n_chunks;
    uint32_t *chunk_cnt, *n_ops;
    uint64_t *chunk_base, *rank;
    unsigned long long* err_key;
};
static void text_takes(svx_takes& t, uint64_t n_bytes, uint32_t n_rec, TextScratch* s) {
    s->n_chunks = n_rec ? (n_bytes + kChunk - 1) / kChunk : 0;  // (text without records: nothing to parse)
    t.add(&s->chunk_cnt, s->n_chunks + 1);
    t.add(&s->chunk_base, s->n_chunks + 1);
    t.add(&s->rank, (size_t)n_rec + 1);
    t.add(&s->err_key, (size_t)n_rec + 1);
    t.add(&s->n_ops, (size_t)n_rec + 1);
}

size_t svx_cigar_text_ws_need(uint64_t n_bytes, uint32_t n_rec) {
    TextScratch s;
    svx_takes t;
    text_takes(t, n_bytes, n_rec, &s);
    return t.bytes();
}

static int text_launch(hipStream_t stream, const uint8_t* d_text, uint64_t n_bytes, const uint64_t* d_rec_off, uint32_t n_rec,
                       uint32_t* d_words, uint64_t cap, uint64_t* d_cigar_off, int32_t* d_ref_len, uint32_t* d_status, const TextScratch& s) {
    const uint64_t n_chunks = s.n_chunks;
    uint32_t *chunk_cnt = s.chunk_cnt, *n_ops = s.n_ops;
    uint64_t *chunk_base = s.chunk_base, *rank = s.rank;
    unsigned long long* err_key = s.err_key;
    hipError_t e = hipMemsetAsync(err_key, 0xFF, ((size_t)n_rec + 1) * 8, stream);
    if (e == hipSuccess && n_rec) e = hipMemsetAsync(d_ref_len, 0, (size_t)n_rec * 4, stream);
    if (e != hipSuccess) return (int)e;
    if (n_chunks) hipLaunchKernelGGL(k_count, dim3((uint32_t)n_chunks), dim3(kThreads), 0, stream, d_text, n_bytes, d_rec_off, n_rec, chunk_cnt, err_key);
    hipLaunchKernelGGL(k_scan, dim3(1), dim3(kScanThreads), 0, stream, chunk_cnt, n_chunks, chunk_base);
    hipLaunchKernelGGL(k_rec_rank, dim3((n_rec + 1 + kWaves - 1) / kWaves), dim3(kThreads), 0, stream, d_text, n_bytes, d_rec_off, n_rec, chunk_base, rank);
    if (n_rec) hipLaunchKernelGGL(k_rec_fin, dim3((n_rec + kThreads - 1) / kThreads), dim3(kThreads), 0, stream, d_text, d_rec_off, n_rec, rank, err_key, d_status, n_ops);
    hipLaunchKernelGGL(k_scan, dim3(1), dim3(kScanThreads), 0, stream, n_ops, (uint64_t)n_rec, d_cigar_off);
    if (n_chunks && n_rec) hipLaunchKernelGGL(k_emit, dim3((uint32_t)n_chunks), dim3(kThreads), 0, stream, d_text, n_bytes, d_rec_off, n_rec, chunk_base, rank, d_status, d_cigar_off, cap, d_words, d_ref_len);
    return (int)hipGetLastError();
}

// The launches on `stream`; d_ws: svx_cigar_text_ws_need bytes, 256-byte aligned.  hipError_t as int.
int svx_cigar_text_parse_on_stream(void* stream, const uint8_t* d_text, uint64_t n_bytes, const uint64_t* d_rec_off, uint32_t n_rec,
                                   uint32_t* d_words, uint64_t cap, uint64_t* d_cigar_off, int32_t* d_ref_len, uint32_t* d_status,
                                   void* d_ws) {
    TextScratch s;
    svx_takes t;
    text_takes(t, n_bytes, n_rec, &s);
    t.place(static_cast<char*>(d_ws), 0);
    return text_launch(static_cast<hipStream_t>(stream), d_text, n_bytes, d_rec_off, n_rec, d_words, cap, d_cigar_off, d_ref_len, d_status, s);
}

extern "C" void svx_sam_register_device_parser(svx_cigar_text_launch_fn, svx_cigar_text_ws_fn);
static const int svx_cigar_text_registered = (svx_sam_register_device_parser(&svx_cigar_text_parse_on_stream, &svx_cigar_text_ws_need), 0);

extern "C" int svx_cigar_text_parse_dev(svx_ctx* ctx, const uint8_t* d_text, uint64_t n_bytes, const uint64_t* d_rec_off, uint32_t n_rec,
                                        uint32_t* d_words, uint64_t cap, uint64_t* d_cigar_off, int32_t* d_ref_len, uint32_t* d_status) {
    if (!ctx) return SVX_E_INVALID;
    if (!d_rec_off || !d_cigar_off || (n_bytes && !d_text) || (n_rec && (!d_ref_len || !d_status)) || (cap && !d_words)) {
        SVX_SET_ERR(ctx, "svx_cigar_text_parse_dev: null argument");
        return SVX_E_INVALID;
    }
    if (n_bytes >= (1ull << 40) || cap < n_bytes / 2) {
        SVX_SET_ERR(ctx, "svx_cigar_text_parse_dev: cap must hold n_bytes / 2 words (an operation is two bytes at least)");
        return SVX_E_INVALID;
    }
    SVX_HIP(ctx, hipSetDevice(ctx->device));
    TextScratch s;
    svx_takes ws;
    text_takes(ws, n_bytes, n_rec, &s);
    SVX_TRY(svx_ws_lay(ctx, ws));
    SVX_TRY(svx_timing_begin(ctx));
    SVX_TRY(svx_timing_mark(ctx, 1));
    const int e = text_launch(ctx->stream, d_text, n_bytes, d_rec_off, n_rec, d_words, cap, d_cigar_off, d_ref_len, d_status, s);
    if (e != 0) {
        SVX_SET_ERR(ctx, "svx_cigar_text_parse_dev: launch failed: %s", hipGetErrorString((hipError_t)e));
        return SVX_E_HIP;
    }
    SVX_TRY(svx_timing_mark(ctx, 2));
    return svx_timing_end(ctx);
}
