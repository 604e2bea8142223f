// svx_fasta_gather.hip — the device gather of a bgzip-compressed FASTA's windows (svx_fasta_bgzf.cpp's device path).
//
// The members under a batch's windows are resident in the handle's arena (inflated and checked by svx_inflate.hip); the
// host cuts every window into chunks of at most SVX_FASTA_CHUNK_BASES output bases whose bytes lie in two members at most
// (a, and the next non-empty one b), so a lane picks its source with one comparison.  A workgroup per chunk: lane k of it
// maps base s = s0 + k to its uncompressed byte through the .fai geometry (s / line_bases by a multiply-shift, line ends
// skipped), reads it from member a or b, upper-cases it when asked and writes it to the packed output.  The data are small
// next to the inflate (tens of MB per sample): one byte per lane and step, coalesced on the output side.
#include <hip/hip_runtime.h>

#include "svx_fasta_bgzf.h"
#include "svx_internal.h"

namespace {

constexpr int kThreads = 256;

__global__ void __launch_bounds__(kThreads) k_fasta_gather(const uint8_t* __restrict__ arena, const svx_fasta_chunk* __restrict__ chunks,
                                                          int upper, uint8_t* __restrict__ out) {
    const svx_fasta_chunk c = chunks[blockIdx.x];
    for (uint32_t k = threadIdx.x; k < c.n; k += kThreads) {
        const uint64_t s = c.s0 + k;
        // s < 2^31 and line_bases < 2^31 (the host's condition for magic != 0): exact, and s * magic < 2^63
        const uint64_t q = c.magic ? (s * c.magic) >> c.shift : s / c.line_bases;
        const uint64_t u = c.off + q * c.line_width + (s - q * c.line_bases);
        uint8_t b = u < c.u_b ? arena[c.src_a + (u - c.u_a)] : arena[c.src_b + (u - c.u_b)];
        if (upper && b >= 'a' && b <= 'z') b = (uint8_t)(b - 32);
        out[c.out + k] = b;
    }
}

// The oriented form (svx_fasta_fetch_oriented): the same chunks; lane k of a reversed chunk takes source base s0 + n - 1 - k,
// so the loads run down across the lanes (still inside members a and b) and the stores stay ascending and coalesced.  Every
// byte then goes through the table of its direction — tabs[0..256) as it lies, tabs[256..512) complemented — which the
// workgroup copies to LDS once.  The index differs per lane, so a table in constant memory would be a third vector
// memory load per base; in LDS the gfx950 code is one ds_write_b8 and one s_barrier per workgroup and, per base, the two
// global_load_ubyte and the global_store_byte of k_fasta_gather plus one ds_read_u8 (the chunk arrives by scalar loads).
__global__ void __launch_bounds__(kThreads) k_fasta_gather_oriented(const uint8_t* __restrict__ arena,
                                                                   const svx_fasta_chunk* __restrict__ chunks,
                                                                   const uint8_t* __restrict__ tabs, uint8_t* __restrict__ out) {
    __shared__ uint8_t lut[256];
    const svx_fasta_chunk c = chunks[blockIdx.x];
    lut[threadIdx.x] = tabs[(c.reverse ? 256u : 0u) + threadIdx.x];  // (kThreads == 256: one entry per lane)
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < c.n; k += kThreads) {
        const uint64_t s = c.reverse ? c.s0 + (c.n - 1 - k) : c.s0 + k;
        const uint64_t q = c.magic ? (s * c.magic) >> c.shift : s / c.line_bases;
        const uint64_t u = c.off + q * c.line_width + (s - q * c.line_bases);
        const uint8_t b = u < c.u_b ? arena[c.src_a + (u - c.u_a)] : arena[c.src_b + (u - c.u_b)];
        out[c.out + k] = lut[b];
    }
}
static_assert(kThreads == 256, "k_fasta_gather_oriented fills its 256-entry table with one entry per lane");

int svx_fasta_gather_on_stream(void* stream, const uint8_t* d_arena, const svx_fasta_chunk* d_chunks, uint32_t n_chunks, int upper,
                               uint8_t* d_out) {
    if (n_chunks == 0) return 0;
    hipLaunchKernelGGL(k_fasta_gather, dim3(n_chunks), dim3(kThreads), 0, static_cast<hipStream_t>(stream), d_arena, d_chunks, upper,
                       d_out);
    return (int)hipGetLastError();
}

int svx_fasta_gather_oriented_on_stream(void* stream, const uint8_t* d_arena, const svx_fasta_chunk* d_chunks, uint32_t n_chunks,
                                        const uint8_t* d_tabs, uint8_t* d_out) {
    if (n_chunks == 0) return 0;
    hipLaunchKernelGGL(k_fasta_gather_oriented, dim3(n_chunks), dim3(kThreads), 0, static_cast<hipStream_t>(stream), d_arena, d_chunks,
                       d_tabs, d_out);
    return (int)hipGetLastError();
}

[[maybe_unused]] const int kRegistered =
    (svx_fasta_register_device(&svx_bgzf_inflate_on_stream, &svx_fasta_gather_on_stream, &svx_fasta_gather_oriented_on_stream,
                               &svx_bgzf_inflate_arena_members), 0);

}  // namespace
