// gcn10_context.hip -- the context runtime behind the C ABI of include/gcn10_gpu.h: the error string, init and
// destroy, the memory, stream and event wrappers, the options, and the helpers every other translation unit launches
// through.  No kernel in this file.

#include <hip/hip_runtime.h>
#include <unistd.h>
#include <hip/hip_ext.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <new>

#include "gcn10_gpu.h"
#include "gcn10_device_util.hpp"
#include "gcn10_gpu_internal.hpp"
#include "gcn10_soil_readers.hpp"

using gcn10::as_stream;
using gcn10::fail;
using gcn10::kLut16Bytes;
using gcn10::kLut1Bytes;
using gcn10::use_device;

namespace gcn10 {

thread_local char g_err[512] = "";

int fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}

int use_device(gcn10_gpu_ctx *ctx)
{
    if (!ctx)
        return fail(GCN10_E_INVAL, "null context");
    HIP_TRY(hipSetDevice(ctx->device));
    return GCN10_OK;
}

hipStream_t as_stream(gcn10_gpu_ctx *ctx, gcn10_stream_t s)
{
    return s ? reinterpret_cast<hipStream_t>(s) : ctx->main_stream;
}

int grow_workspace(void **ws, size_t *cap, size_t need)
{
    if (need <= *cap)
        return GCN10_OK;
    HIP_TRY(hipDeviceSynchronize());            // the old workspace may still be in use
    if (*ws)
        HIP_TRY(hipFree(*ws));
    *ws = nullptr;
    *cap = 0;
    HIP_TRY(hipMalloc(ws, need));
    *cap = need;
    return GCN10_OK;
}

uint32_t grid_cap(const gcn10_gpu_ctx *ctx, int per_cu)
{
    return (uint32_t)(ctx->n_cus > 0 ? ctx->n_cus : 256) * (uint32_t)per_cu;
}

uint32_t stream_grid(const gcn10_gpu_ctx *ctx, uint64_t nchunks, int blocks_per_cu)
{
    uint64_t cap = (uint64_t)ctx->n_cus * (blocks_per_cu > 0 ? blocks_per_cu : ctx->opt.grid_blocks_per_cu);
    cap -= cap % 8u;
    if (cap < 8)
        cap = 8;
    uint64_t g = nchunks < cap ? nchunks : cap;
    return (uint32_t)(g ? g : 1);
}

hipError_t launch_timed(gcn10_gpu_ctx *ctx, const void *fn, uint32_t grid, void **args, hipStream_t s)
{
    if (!ctx->time_start || !ctx->time_stop)
        return hipLaunchKernel(fn, dim3(grid), dim3(kThreads), args, 0, s);
    const hipError_t e = hipExtLaunchKernel(fn, dim3(grid), dim3(kThreads), args, 0, s, ctx->time_start,
                                            ctx->time_stop, 0);
    if (e == hipSuccess)
        ctx->time_start = ctx->time_stop = nullptr;
    return e;
}

}  // namespace gcn10

namespace {

// ---- the options of gcn10_gpu_set_option: name, member of gcn10_gpu_ctx::Options, accepted values ----
template <int LO, int HI>
bool between(int v)
{
    return v >= LO && v <= HI;
}

struct Option {
    const char *name;
    int gcn10_gpu_ctx::Options::*field;
    bool (*accepts)(int);
};

typedef gcn10_gpu_ctx::Options Opt;
const Option kOptions[] = {
    { "grid_blocks_per_cu", &Opt::grid_blocks_per_cu, between<1, 64> },
    { "ilp16", &Opt::ilp16, between<0, 2> },
    { "ilp1", &Opt::ilp1, [](int v) { return v == 1 || v == 2 || v == 4; } },
    { "nontemporal", &Opt::nontemporal, between<0, 1> },
    { "xcd_slabs", &Opt::xcd_slabs, between<0, 1> },
    { "deflate_wave_codes", &Opt::deflate_wave_codes, between<0, 1> },
    { "arena_segment_align", &Opt::arena_segment_align, [](int v) { return between<16, 4096>(v) && (v & (v - 1)) == 0; } },
    { "fused_emit", &Opt::fused_emit, between<0, 1> },
    { "fused_parse", &Opt::fused_parse, between<0, 1> },
    { "event_sync_sleep_us", &Opt::event_sync_sleep_us, between<0, 100000> },
    { "prefetch", &Opt::prefetch, between<-1, 1> },
    { "compact_soil", &Opt::compact_soil, between<0, 1> },     // strips launched from now on (every prepared tile has the tables)
};

}  // namespace

// ------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------
extern "C" {

int gcn10_gpu_abi_version(void)
{
    return GCN10_GPU_ABI_VERSION;
}

const char *gcn10_gpu_last_error(void)
{
    return gcn10::g_err;
}

int gcn10_gpu_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess)
        return 0;
    return n;
}

int gcn10_gpu_init(int device, gcn10_gpu_ctx **out)
{
    if (!out)
        return fail(GCN10_E_INVAL, "gcn10_gpu_init: null out pointer");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(GCN10_E_NODEVICE, "no HIP device visible (%s); this engine has no CPU fallback",
                    e != hipSuccess ? hipGetErrorString(e) : "device count 0");
    if (device < 0 || device >= n)
        return fail(GCN10_E_INVAL, "device %d out of range (0..%d)", device, n - 1);
    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(GCN10_E_NODEVICE, "device %d is %s; this library carries gfx950 code only",
                    device, prop.gcnArchName);

    gcn10_gpu_ctx *ctx = new (std::nothrow) gcn10_gpu_ctx();
    if (!ctx)
        return fail(GCN10_E_NOMEM, "context allocation failed");
    ctx->device = device;
    ctx->n_cus = prop.multiProcessorCount;
    hipError_t e2 = hipStreamCreateWithFlags(&ctx->main_stream, hipStreamNonBlocking);
    if (e2 == hipSuccess)
        e2 = hipMalloc(reinterpret_cast<void **>(&ctx->d_lut16), kLut16Bytes);
    if (e2 == hipSuccess)
        e2 = hipMalloc(reinterpret_cast<void **>(&ctx->d_lut1), GCN10_N_TABLES * kLut1Bytes);
    // the "complex tile" word lives as long as the context: generation numbers never repeat within its life
    if (e2 == hipSuccess)
        e2 = hipMalloc(reinterpret_cast<void **>(&ctx->tile.d_soil_complex), 16);
    if (e2 == hipSuccess)
        e2 = hipMemset(ctx->tile.d_soil_complex, 0, 16);
    if (e2 == hipSuccess)
        e2 = hipEventCreateWithFlags(&ctx->tile.hx_made_ev, hipEventDisableTiming);
    if (e2 != hipSuccess) {
        int rc = fail(GCN10_E_HIP, "context setup: %s", hipGetErrorString(e2));
        gcn10_gpu_destroy(ctx);
        return rc;
    }
    *out = ctx;
    return GCN10_OK;
}

void gcn10_gpu_destroy(gcn10_gpu_ctx *ctx)
{
    if (!ctx)
        return;
    (void)hipSetDevice(ctx->device);
    if (ctx->main_stream) {
        (void)hipStreamSynchronize(ctx->main_stream);
        (void)hipStreamDestroy(ctx->main_stream);
    }
    if (ctx->d_lut16)
        (void)hipFree(ctx->d_lut16);
    if (ctx->d_lut1)
        (void)hipFree(ctx->d_lut1);
    if (ctx->d_wlut)
        (void)hipFree(ctx->d_wlut);
    if (ctx->d_rain_tables)
        (void)hipFree(ctx->d_rain_tables);
    if (ctx->tile.d_hx_alloc)
        (void)hipFree(ctx->tile.d_hx_alloc);
    if (ctx->tile.d_soil_complex)
        (void)hipFree(ctx->tile.d_soil_complex);
    if (ctx->tile.hx_made_ev)
        (void)hipEventDestroy(ctx->tile.hx_made_ev);
    if (ctx->ws.deflate)
        (void)hipFree(ctx->ws.deflate);
    if (ctx->ws.inflate)
        (void)hipFree(ctx->ws.inflate);
    if (ctx->ws.lzw)
        (void)hipFree(ctx->ws.lzw);
    if (ctx->ws.cell_tables)
        (void)hipFree(ctx->ws.cell_tables);
    if (ctx->d_cell_byte_tables)
        (void)hipFree(ctx->d_cell_byte_tables);
    if (ctx->d_class_of)
        (void)hipFree(ctx->d_class_of);
    delete ctx;
}

int gcn10_gpu_device_info(gcn10_gpu_ctx *ctx, char *name, size_t cap, size_t *hbm_bytes)
{
    int rc = use_device(ctx);
    if (rc)
        return rc;
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, ctx->device));
    if (name && cap)
        snprintf(name, cap, "%s (%s)", prop.name[0] ? prop.name : "AMD GPU", prop.gcnArchName);
    if (hbm_bytes)
        *hbm_bytes = prop.totalGlobalMem;
    return prop.multiProcessorCount;
}

int gcn10_gpu_pci_bus_id(int device, char *buf, size_t cap)
{
    if (!buf || cap < 13)
        return fail(GCN10_E_INVAL, "gcn10_gpu_pci_bus_id: buffer too small");
    HIP_TRY(hipDeviceGetPCIBusId(buf, (int)cap, device));
    return GCN10_OK;
}

// ---- memory / streams / events ------------------------------------------

int gcn10_gpu_malloc(gcn10_gpu_ctx *ctx, size_t bytes, void **dptr)
{
    int rc = use_device(ctx);
    if (rc)
        return rc;
    if (!dptr)
        return fail(GCN10_E_INVAL, "gcn10_gpu_malloc: null out pointer");
    *dptr = nullptr;
    HIP_TRY(hipMalloc(dptr, bytes ? bytes : 1));
    return GCN10_OK;
}

int gcn10_gpu_free(gcn10_gpu_ctx *ctx, void *dptr)
{
    int rc = use_device(ctx);
    if (rc)
        return rc;
    if (dptr)
        HIP_TRY(hipFree(dptr));
    return GCN10_OK;
}

int gcn10_gpu_host_alloc(gcn10_gpu_ctx *ctx, size_t bytes, void **hptr)
{
    int rc = use_device(ctx);
    if (rc)
        return rc;
    if (!hptr)
        return fail(GCN10_E_INVAL, "gcn10_gpu_host_alloc: null out pointer");
    *hptr = nullptr;
    HIP_TRY(hipHostMalloc(hptr, bytes ? bytes : 1, hipHostMallocDefault));
    return GCN10_OK;
}

int gcn10_gpu_host_free(gcn10_gpu_ctx *ctx, void *hptr)
{
    int rc = use_device(ctx);
    if (rc)
        return rc;
    if (hptr)
        HIP_TRY(hipHostFree(hptr));
    return GCN10_OK;
}

int gcn10_gpu_memcpy_h2d(gcn10_gpu_ctx *ctx, void *dst, const void *src, size_t bytes,
                         gcn10_stream_t stream)
{
    int rc = use_device(ctx);
    if (rc)
        return rc;
    if (bytes && (!dst || !src))
        return fail(GCN10_E_INVAL, "gcn10_gpu_memcpy_h2d: null pointer");
    if (bytes)
        HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, as_stream(ctx, stream)));
    return GCN10_OK;
}

int gcn10_gpu_memcpy_d2h(gcn10_gpu_ctx *ctx, void *dst, const void *src, size_t bytes,
                         gcn10_stream_t stream)
{
    int rc = use_device(ctx);
    if (rc)
        return rc;
    if (bytes && (!dst || !src))
        return fail(GCN10_E_INVAL, "gcn10_gpu_memcpy_d2h: null pointer");
    if (bytes)
        HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, as_stream(ctx, stream)));
    return GCN10_OK;
}

int gcn10_gpu_memset(gcn10_gpu_ctx *ctx, void *dptr, int value, size_t bytes,
                     gcn10_stream_t stream)
{
    int rc = use_device(ctx);
    if (rc)
        return rc;
    if (bytes && !dptr)
        return fail(GCN10_E_INVAL, "gcn10_gpu_memset: null pointer");
    if (bytes)
        HIP_TRY(hipMemsetAsync(dptr, value, bytes, as_stream(ctx, stream)));
    return GCN10_OK;
}

int gcn10_gpu_stream_create(gcn10_gpu_ctx *ctx, gcn10_stream_t *stream)
{
    int rc = use_device(ctx);
    if (rc)
        return rc;
    if (!stream)
        return fail(GCN10_E_INVAL, "gcn10_gpu_stream_create: null out pointer");
    hipStream_t s = nullptr;
    HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    *stream = s;
    return GCN10_OK;
}

int gcn10_gpu_stream_destroy(gcn10_gpu_ctx *ctx, gcn10_stream_t stream)
{
    int rc = use_device(ctx);
    if (rc)
        return rc;
    if (stream)
        HIP_TRY(hipStreamDestroy(reinterpret_cast<hipStream_t>(stream)));
    return GCN10_OK;
}

int gcn10_gpu_stream_sync(gcn10_gpu_ctx *ctx, gcn10_stream_t stream)
{
    int rc = use_device(ctx);
    if (rc)
        return rc;
    HIP_TRY(hipStreamSynchronize(as_stream(ctx, stream)));
    return GCN10_OK;
}

int gcn10_gpu_device_sync(gcn10_gpu_ctx *ctx)
{
    int rc = use_device(ctx);
    if (rc)
        return rc;
    HIP_TRY(hipDeviceSynchronize());
    return GCN10_OK;
}

int gcn10_gpu_event_create(gcn10_gpu_ctx *ctx, gcn10_event_t *ev)
{
    int rc = use_device(ctx);
    if (rc)
        return rc;
    if (!ev)
        return fail(GCN10_E_INVAL, "gcn10_gpu_event_create: null out pointer");
    hipEvent_t e = nullptr;
    HIP_TRY(hipEventCreate(&e));
    *ev = e;
    return GCN10_OK;
}

int gcn10_gpu_event_destroy(gcn10_gpu_ctx *ctx, gcn10_event_t ev)
{
    int rc = use_device(ctx);
    if (rc)
        return rc;
    if (ev)
        HIP_TRY(hipEventDestroy(reinterpret_cast<hipEvent_t>(ev)));
    return GCN10_OK;
}

int gcn10_gpu_event_record(gcn10_gpu_ctx *ctx, gcn10_event_t ev, gcn10_stream_t stream)
{
    int rc = use_device(ctx);
    if (rc)
        return rc;
    if (!ev)
        return fail(GCN10_E_INVAL, "gcn10_gpu_event_record: null event");
    HIP_TRY(hipEventRecord(reinterpret_cast<hipEvent_t>(ev), as_stream(ctx, stream)));
    return GCN10_OK;
}

int gcn10_gpu_event_sync(gcn10_gpu_ctx *ctx, gcn10_event_t ev)
{
    int rc = use_device(ctx);
    if (rc)
        return rc;
    if (!ev)
        return fail(GCN10_E_INVAL, "gcn10_gpu_event_sync: null event");
    if (ctx->opt.event_sync_sleep_us > 0) {
        // a waiter that sleeps between queries: hipEventSynchronize spins in user mode for the whole wait, which is
        // what a timing loop wants and what a thread of a CPU-quota-bound host pipeline does not (the threads that
        // wait for a strip's bytes burnt 18 % of the program's CPU time: profiles/r03/host_cpu_by_thread_and_job.txt)
        for (;;) {
            const hipError_t e = hipEventQuery(reinterpret_cast<hipEvent_t>(ev));
            if (e == hipSuccess)
                break;
            if (e != hipErrorNotReady)
                HIP_TRY(e);
            usleep((useconds_t)ctx->opt.event_sync_sleep_us);
        }
        return GCN10_OK;
    }
    HIP_TRY(hipEventSynchronize(reinterpret_cast<hipEvent_t>(ev)));
    return GCN10_OK;
}

int gcn10_gpu_stream_wait_event(gcn10_gpu_ctx *ctx, gcn10_stream_t stream, gcn10_event_t ev)
{
    int rc = use_device(ctx);
    if (rc)
        return rc;
    if (!ev)
        return fail(GCN10_E_INVAL, "gcn10_gpu_stream_wait_event: null event");
    HIP_TRY(hipStreamWaitEvent(as_stream(ctx, stream), reinterpret_cast<hipEvent_t>(ev), 0));
    return GCN10_OK;
}

int gcn10_gpu_event_elapsed_ms(gcn10_gpu_ctx *ctx, gcn10_event_t start, gcn10_event_t stop,
                               float *ms)
{
    int rc = use_device(ctx);
    if (rc)
        return rc;
    if (!start || !stop || !ms)
        return fail(GCN10_E_INVAL, "gcn10_gpu_event_elapsed_ms: null argument");
    HIP_TRY(hipEventElapsedTime(ms, reinterpret_cast<hipEvent_t>(start),
                                reinterpret_cast<hipEvent_t>(stop)));
    return GCN10_OK;
}

int gcn10_gpu_set_option(gcn10_gpu_ctx *ctx, const char *name, int value)
{
    if (!ctx || !name)
        return fail(GCN10_E_INVAL, "gcn10_gpu_set_option: null argument");
    if (!strcmp(name, "defaults")) {
        ctx->opt = gcn10_gpu_ctx::Options();
        return GCN10_OK;
    }
    for (const Option &o : kOptions) {
        if (strcmp(name, o.name) || !o.accepts(value))
            continue;
        ctx->opt.*o.field = value;
        if (o.field == &gcn10_gpu_ctx::Options::ilp1)
            ctx->opt.single.set = false;        // an explicit setting replaces a calibrated shape
        return GCN10_OK;
    }
    return fail(GCN10_E_INVAL, "gcn10_gpu_set_option: unknown option or bad value: %s=%d", name, value);
}

int gcn10_gpu_time_next_strip(gcn10_gpu_ctx *ctx, gcn10_event_t start, gcn10_event_t stop)
{
    if (!ctx || !start || !stop)
        return fail(GCN10_E_INVAL, "gcn10_gpu_time_next_strip: null argument");
    ctx->time_start = reinterpret_cast<hipEvent_t>(start);
    ctx->time_stop = reinterpret_cast<hipEvent_t>(stop);
    return GCN10_OK;
}

const char *gcn10_gpu_last_kernel_name(gcn10_gpu_ctx *ctx)
{
    return ctx ? ctx->last_kernel : "";
}

}  // extern "C"
