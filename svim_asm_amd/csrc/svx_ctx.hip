// svx_ctx.hip — context lifecycle, workspace, timing.  Part of libsvx.so (C-ABI in include/svx.h).
#include "svx_internal.h"

extern "C" const char* svx_version(void) { return "svx 0.1.0 (gfx950)"; }

extern "C" int svx_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

extern "C" int svx_device_pci_bus_id(int device, char* out, int len) {
    if (!out || len < 16) return SVX_E_INVALID;
    out[0] = 0;
    if (hipDeviceGetPCIBusId(out, len, device) != hipSuccess) {
        (void)hipGetLastError();
        return SVX_E_NODEVICE;
    }
    return SVX_OK;
}

static int ctx_create_common(int device, void* stream, bool own, svx_ctx** out) {
    if (!out) return SVX_E_INVALID;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return SVX_E_NODEVICE;
    if (device < 0 || device >= n) return SVX_E_NODEVICE;
    if (hipSetDevice(device) != hipSuccess) return SVX_E_HIP;
    svx_ctx* c = new (std::nothrow) svx_ctx();
    if (!c) return SVX_E_NOMEM;
    c->device = device;
    if (own) {
        if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
            delete c;
            return SVX_E_HIP;
        }
        c->own_stream = true;
    } else {
        c->stream = reinterpret_cast<hipStream_t>(stream);
        c->own_stream = false;
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0)
        c->n_cu = prop.multiProcessorCount;
    *out = c;
    return SVX_OK;
}

extern "C" int svx_ctx_create(int device, svx_ctx** out) {
    return ctx_create_common(device, nullptr, true, out);
}
extern "C" int svx_ctx_create_on_stream(int device, void* hip_stream, svx_ctx** out) {
    return ctx_create_common(device, hip_stream, false, out);
}

extern "C" void svx_ctx_destroy(svx_ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    if (ctx->ws) (void)hipFree(ctx->ws);
    if (ctx->stage) (void)hipFree(ctx->stage);
    if (ctx->hpin) (void)hipHostFree(ctx->hpin);
    for (int i = 0; i < 4; ++i)
        if (ctx->ev[i]) (void)hipEventDestroy(ctx->ev[i]);
    if (ctx->ev_dom) (void)hipEventDestroy(ctx->ev_dom);
    if (ctx->ev_block) (void)hipEventDestroy(ctx->ev_block);
    if (ctx->own_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

extern "C" int svx_ctx_sync(svx_ctx* ctx) {
    if (!ctx) return SVX_E_INVALID;
    SVX_HIP(ctx, hipSetDevice(ctx->device));
    SVX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return svx_barrier_check(ctx);
}

int svx_barrier_check(svx_ctx* ctx) {
    if (!ctx->barrier_pending || !ctx->ws) return SVX_OK;
    ctx->barrier_pending = false;
    uint32_t note = 0;
    SVX_HIP(ctx, hipMemcpy(&note, ctx->ws + 4 * SVX_WS_BARRIER_NOTE_WORD, 4, hipMemcpyDeviceToHost));
    if (!note) return SVX_OK;
    SVX_HIP(ctx, hipMemset(ctx->ws, 0, 4096));  // counters of the broken launch included
    ctx->pair_launches = 0;
    ctx->barrier_timed_out = true;  // svx_ctx_barrier_timed_out: the caller of a _dev entry may re-enqueue wait-free
    SVX_SET_ERR(ctx, "svx_pair_partition: a wait between workgroups ran out (more than four contexts sorting on one "
                     "device?); the results of that call are invalid");
    return SVX_E_HIP;
}

extern "C" const char* svx_last_error(const svx_ctx* ctx) { return ctx ? ctx->err : "null context"; }

static int grow(svx_ctx* ctx, char** buf, size_t* have, size_t want) {
    if (want <= *have) return SVX_OK;
    SVX_HIP(ctx, hipSetDevice(ctx->device));
    // earlier work on the stream may still use the old buffer
    SVX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (*buf) {
        SVX_HIP(ctx, hipFree(*buf));
        *buf = nullptr;
        *have = 0;
    }
    size_t sz = svx_align_up(want + want / 8, 1 << 20);
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, sz);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        SVX_SET_ERR(ctx, "hipMalloc(%zu) failed: %s", sz, hipGetErrorString(e));
        return SVX_E_NOMEM;
    }
    *buf = static_cast<char*>(p);
    *have = sz;
    // kernels keep self-cleaning counters at the start of the workspace: they start out as zero
    SVX_HIP(ctx, hipMemsetAsync(p, 0, 4096, ctx->stream));
    return SVX_OK;
}

int svx_ws_reserve(svx_ctx* ctx, size_t total) {
    if (ctx->barrier_pending && total + 4096 > ctx->ws_bytes) {  // the note would go away with the old buffer
        SVX_HIP(ctx, hipSetDevice(ctx->device));
        SVX_HIP(ctx, hipStreamSynchronize(ctx->stream));
        SVX_TRY(svx_barrier_check(ctx));
    }
    // the first 4 KiB of the workspace are a header of self-cleaning counters (zeroed at
    // allocation, left at zero by the kernels that use them); per-call scratch starts after it
    ctx->ws_used = 4096;
    return grow(ctx, &ctx->ws, &ctx->ws_bytes, total + 4096);
}
int svx_wait_blocking(svx_ctx* ctx) {
    SVX_HIP(ctx, hipSetDevice(ctx->device));
    if (!ctx->ev_block) SVX_HIP(ctx, hipEventCreateWithFlags(&ctx->ev_block, hipEventBlockingSync | hipEventDisableTiming));
    SVX_HIP(ctx, hipEventRecord(ctx->ev_block, ctx->stream));
    SVX_HIP(ctx, hipEventSynchronize(ctx->ev_block));
    return SVX_OK;
}
int svx_stage_reserve(svx_ctx* ctx, size_t total) {
    ctx->stage_used = 0;
    return grow(ctx, &ctx->stage, &ctx->stage_bytes, total);
}

// Test facility (include/svx.h, "the scratch contract"): plain memsets and one copy, no kernel.
extern "C" int svx_ctx_scratch_fill(svx_ctx* ctx, int byte) {
    if (!ctx) return SVX_E_INVALID;
    const int b = byte & 0xFF;
    SVX_HIP(ctx, hipSetDevice(ctx->device));
    SVX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->ws && ctx->ws_bytes > 4096) SVX_HIP(ctx, hipMemset(ctx->ws + 4096, b, ctx->ws_bytes - 4096));
    if (ctx->stage && ctx->stage_bytes) SVX_HIP(ctx, hipMemset(ctx->stage, b, ctx->stage_bytes));
    if (ctx->hpin && ctx->hpin_bytes) memset(ctx->hpin, b, ctx->hpin_bytes);
    SVX_HIP(ctx, hipDeviceSynchronize());  // hipMemset may return before the device has finished it
    SVX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SVX_OK;
}

extern "C" int svx_ctx_scratch_header(svx_ctx* ctx, uint32_t out[1024]) {
    if (!ctx || !out) return SVX_E_INVALID;
    SVX_HIP(ctx, hipSetDevice(ctx->device));
    SVX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    memset(out, 0, 4096);
    if (ctx->ws) SVX_HIP(ctx, hipMemcpy(out, ctx->ws, 4096, hipMemcpyDeviceToHost));
    return SVX_OK;
}

extern "C" int svx_ctx_set_small_batch_ops(svx_ctx* ctx, uint64_t max_ops) {
    if (!ctx) return SVX_E_INVALID;
    ctx->small_batch_ops = max_ops > (1ull << 23) ? (1ull << 23) : max_ops;  // the limit include/svx.h states
    return SVX_OK;
}

extern "C" int svx_ctx_barrier_timed_out(svx_ctx* ctx) {
    if (!ctx) return 0;
    const bool was = ctx->barrier_timed_out;
    ctx->barrier_timed_out = false;
    return was ? 1 : 0;
}

extern "C" int svx_ctx_set_split_chain(svx_ctx* ctx, int on) {
    if (!ctx) return SVX_E_INVALID;
    ctx->split_chain = on != 0;
    return SVX_OK;
}

extern "C" int svx_ctx_set_pair_single_launch_max(svx_ctx* ctx, uint32_t max_candidates) {
    if (!ctx) return SVX_E_INVALID;
    ctx->pair_single_max = max_candidates > 131072u ? 131072u : max_candidates;
    return SVX_OK;
}

extern "C" int svx_ctx_set_edit_wavefront_cap(svx_ctx* ctx, uint32_t max_edits) {
    if (!ctx) return SVX_E_INVALID;
    ctx->wfa_cap = max_edits > 4096u ? 4096u : max_edits;
    return SVX_OK;
}

extern "C" int svx_dev_malloc(svx_ctx* ctx, size_t bytes, void** d_out) {
    if (!ctx || !d_out) return SVX_E_INVALID;
    *d_out = nullptr;
    SVX_HIP(ctx, hipSetDevice(ctx->device));
    hipError_t e = hipMalloc(d_out, bytes ? bytes : 1);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        SVX_SET_ERR(ctx, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
        return SVX_E_NOMEM;
    }
    return SVX_OK;
}

extern "C" int svx_dev_free(svx_ctx* ctx, void* d_ptr) {
    if (!ctx) return SVX_E_INVALID;
    if (!d_ptr) return SVX_OK;
    SVX_HIP(ctx, hipSetDevice(ctx->device));
    SVX_HIP(ctx, hipStreamSynchronize(ctx->stream));  // kernels on the stream may still use it
    SVX_HIP(ctx, hipFree(d_ptr));
    return SVX_OK;
}

extern "C" int svx_dev_upload(svx_ctx* ctx, void* d_dst, const void* src, size_t bytes) {
    if (!ctx || (bytes && (!d_dst || !src))) return SVX_E_INVALID;
    if (!bytes) return SVX_OK;
    SVX_HIP(ctx, hipSetDevice(ctx->device));
    SVX_HIP(ctx, hipMemcpyAsync(d_dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    // pageable source: the copy is staged before the call returns, `src` may be reused
    return SVX_OK;
}

extern "C" int svx_dev_download(svx_ctx* ctx, void* dst, const void* d_src, size_t bytes) {
    if (!ctx || (bytes && (!dst || !d_src))) return SVX_E_INVALID;
    SVX_HIP(ctx, hipSetDevice(ctx->device));
    if (bytes) SVX_HIP(ctx, hipMemcpyAsync(dst, d_src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    SVX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SVX_OK;
}

extern "C" int svx_ctx_wait_dominant(svx_ctx* ctx, svx_ctx* other) {
    if (!ctx || !other) return SVX_E_INVALID;
    if (ctx->device != other->device) {
        SVX_SET_ERR(ctx, "svx_ctx_wait_dominant: contexts live on different devices");
        return SVX_E_INVALID;
    }
    other->want_dom = true;  // from now on `other` records an event after its streaming kernel
    if (!other->ev_dom_recorded) return SVX_OK;
    SVX_HIP(ctx, hipSetDevice(ctx->device));
    SVX_HIP(ctx, hipStreamWaitEvent(ctx->stream, other->ev_dom, 0));
    return SVX_OK;
}

extern "C" int svx_ctx_set_timing(svx_ctx* ctx, int enabled) {
    if (!ctx) return SVX_E_INVALID;
    SVX_HIP(ctx, hipSetDevice(ctx->device));
    if (enabled && !ctx->ev[0]) {
        for (int i = 0; i < 4; ++i) SVX_HIP(ctx, hipEventCreate(&ctx->ev[i]));
    }
    ctx->timing = enabled != 0;
    ctx->ev_valid = false;
    return SVX_OK;
}

int svx_timing_begin(svx_ctx* ctx) {
    if (!ctx->timing) return SVX_OK;
    ctx->ev_valid = false;
    SVX_HIP(ctx, hipEventRecord(ctx->ev[0], ctx->stream));
    return SVX_OK;
}
int svx_timing_mark(svx_ctx* ctx, int which) {
    if (!ctx->timing) return SVX_OK;
    SVX_HIP(ctx, hipEventRecord(ctx->ev[which], ctx->stream));
    return SVX_OK;
}
int svx_timing_end(svx_ctx* ctx) {
    if (!ctx->timing) return SVX_OK;
    SVX_HIP(ctx, hipEventRecord(ctx->ev[3], ctx->stream));
    ctx->ev_valid = true;
    return SVX_OK;
}

extern "C" int svx_ctx_last_kernel_ms(svx_ctx* ctx, float* ms_total, float* ms_dominant) {
    if (!ctx) return SVX_E_INVALID;
    if (!ctx->timing || !ctx->ev_valid) {
        SVX_SET_ERR(ctx, "no timed call recorded (svx_ctx_set_timing(ctx,1) then a *_dev call)");
        return SVX_E_INVALID;
    }
    SVX_HIP(ctx, hipSetDevice(ctx->device));
    SVX_HIP(ctx, hipEventSynchronize(ctx->ev[3]));
    float t = 0.f, d = 0.f;
    SVX_HIP(ctx, hipEventElapsedTime(&t, ctx->ev[0], ctx->ev[3]));
    SVX_HIP(ctx, hipEventElapsedTime(&d, ctx->ev[1], ctx->ev[2]));
    if (ms_total) *ms_total = t;
    if (ms_dominant) *ms_dominant = d;
    return SVX_OK;
}

namespace {
typedef uint32_t probe_u32x4 __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(256) void k_hbm_read_probe(const probe_u32x4* __restrict__ in, size_t n_u4, uint32_t* out) {
    const size_t per_block = 256 * 4;
    uint32_t acc = 0;
    for (size_t base = (size_t)blockIdx.x * per_block; base < n_u4; base += (size_t)gridDim.x * per_block) {
        probe_u32x4 v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const size_t i = base + (size_t)k * 256 + threadIdx.x;
            v[k] = i < n_u4 ? __builtin_nontemporal_load(in + i) : probe_u32x4{0, 0, 0, 0};
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) acc ^= v[k].x ^ v[k].y ^ v[k].z ^ v[k].w;
    }
    if (acc == 0x12345678u) out[0] = acc;  // practically never: keeps the loads alive
}
}  // namespace

extern "C" int svx_hbm_read_probe_dev(svx_ctx* ctx, const void* d_buf, size_t bytes, uint32_t reps, float* ms_per_pass) {
    if (!ctx || !d_buf || !ms_per_pass || bytes < 16 || reps == 0 || (reinterpret_cast<uintptr_t>(d_buf) & 15u)) return SVX_E_INVALID;
    SVX_HIP(ctx, hipSetDevice(ctx->device));
    uint32_t* d_out;
    svx_takes ws;
    ws.add(&d_out, 4);
    SVX_TRY(svx_ws_lay(ctx, ws));
    const size_t n = bytes / 16;
    const size_t blocks = (n + 1023) / 1024;
    const dim3 grid((unsigned)(blocks < 102400 ? blocks : 102400));
    hipEvent_t a, b;
    SVX_HIP(ctx, hipEventCreate(&a));
    SVX_HIP(ctx, hipEventCreate(&b));
    hipLaunchKernelGGL(k_hbm_read_probe, grid, dim3(256), 0, ctx->stream, static_cast<const probe_u32x4*>(d_buf), n, d_out);
    SVX_HIP(ctx, hipEventRecord(a, ctx->stream));
    for (uint32_t r = 0; r < reps; ++r)
        hipLaunchKernelGGL(k_hbm_read_probe, grid, dim3(256), 0, ctx->stream, static_cast<const probe_u32x4*>(d_buf), n, d_out);
    SVX_HIP(ctx, hipEventRecord(b, ctx->stream));
    SVX_HIP(ctx, hipEventSynchronize(b));
    float ms = 0.f;
    SVX_HIP(ctx, hipEventElapsedTime(&ms, a, b));
    (void)hipEventDestroy(a);
    (void)hipEventDestroy(b);
    *ms_per_pass = ms / (float)reps;
    return SVX_OK;
}
