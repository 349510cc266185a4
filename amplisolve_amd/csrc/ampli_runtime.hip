// amplisolve_amd/csrc/ampli_runtime.hip -- the context and runtime plumbing of libamplisolve_hip.so: context create / destroy, error
// strings, device probe, the asynchronous drain's join, position ranges on concurrent streams, hipGraph capture, memory, copies,
// events and the ampli_set_* knobs.  The kernels and their launchers are in ampli_kernels.hip and the units
// its header comment maps; ampli_internal.h declares what the launchers use of this file.
#include <cstdio>
#include <algorithm>
#include <new>

#include "ampli_internal.h"

extern "C" int ampli_abi_version(void) { return AMPLI_ABI_VERSION; }

extern "C" const char *ampli_strerror(int code)
{
    switch (code) {
    case AMPLI_OK: return "ok";
    case AMPLI_E_INVALID: return "invalid argument";
    case AMPLI_E_HIP: return "HIP runtime error (no MI355X visible, or a call failed)";
    case AMPLI_E_NOMEM: return "out of memory";
    case AMPLI_E_ENVELOPE: return "accumulators left the exactness envelope";
    case AMPLI_E_CAPACITY: return "call list capacity exceeded";
    case AMPLI_E_RANGE: return "count outside the integer envelope (>= 2^24)";
    case AMPLI_E_COMM_TIMEOUT: return "RCCL communicator start-up timed out (the process must end)";
    default: return "unknown error";
    }
}

extern "C" int ampli_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// the same, saying WHY when there is nothing to count: the number of devices, or -1 with hipGetDeviceCount's own error
// name and text in msg ("hipErrorNoDevice: no ROCm-capable device is detected")
extern "C" int ampli_device_probe(char *msg, size_t cap)
{
    int n = 0;
    const hipError_t e = hipGetDeviceCount(&n);
    if (msg && cap) msg[0] = 0;
    if (e == hipSuccess) return n;
    (void)hipGetLastError(); // do not leave the error behind for the next call's check
    if (msg && cap) snprintf(msg, cap, "%s: %s", hipGetErrorName(e), hipGetErrorString(e));
    return -1;
}

extern "C" int ampli_ctx_create(int device_ordinal, void *stream, ampli_ctx **out)
{
    if (!out) return AMPLI_E_INVALID;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return AMPLI_E_HIP;
    if (device_ordinal < 0 || device_ordinal >= n) return AMPLI_E_INVALID;
    ampli_ctx *ctx = new (std::nothrow) ampli_ctx();
    if (!ctx) return AMPLI_E_NOMEM;
    ctx->device = device_ordinal;
    if (hipSetDevice(device_ordinal) != hipSuccess) { delete ctx; return AMPLI_E_HIP; }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_ordinal) == hipSuccess) ctx->n_cu = prop.multiProcessorCount;
    if (stream == AMPLI_STREAM_OWN) {
        if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) { delete ctx; return AMPLI_E_HIP; }
        ctx->own_stream = true;
    } else {
        ctx->stream = (hipStream_t)stream; // NULL = the device's default (null) stream
    }
    if (hipMalloc((void **)&ctx->d_flags, 256) != hipSuccess || hipMemset(ctx->d_flags, 0, 256) != hipSuccess) {
        if (ctx->own_stream) (void)hipStreamDestroy(ctx->stream);
        delete ctx;
        return AMPLI_E_NOMEM;
    }
    *out = ctx;
    return AMPLI_OK;
}

extern "C" void ampli_ctx_destroy(ampli_ctx *ctx)
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->ws) (void)hipFree(ctx->ws);
    if (ctx->d_flags) (void)hipFree(ctx->d_flags);
    for (int k = 0; k < AMPLI_MAX_RANGES; ++k) {
        AmpliLane &l = ctx->lanes[k];
        if (l.stream) { (void)hipStreamSynchronize(l.stream); (void)hipStreamDestroy(l.stream); }
        if (l.q.items) (void)hipFree(l.q.items);
        if (l.q.n) (void)hipFree(l.q.n);
        if (l.done) (void)hipEventDestroy(l.done);
    }
    if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
    if (ctx->d_lgtab) (void)hipFree(ctx->d_lgtab);
    if (ctx->d_limit_stats) (void)hipFree(ctx->d_limit_stats);
    if (ctx->d_power_stats) (void)hipFree(ctx->d_power_stats);
    if (ctx->side) { (void)hipStreamSynchronize(ctx->side); (void)hipStreamDestroy(ctx->side); }
    if (ctx->ev_stream_done) (void)hipEventDestroy(ctx->ev_stream_done);
    if (ctx->ev_drain_done) (void)hipEventDestroy(ctx->ev_drain_done);
    if (ctx->own_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

extern "C" const char *ampli_last_error(ampli_ctx *ctx) { return ctx ? ctx->err.c_str() : "no context"; }
extern "C" void *ampli_stream(ampli_ctx *ctx) { return ctx ? (void *)main_stream(ctx) : nullptr; }

// main stream waits for the drain kernel still running on the side stream (no host block)
int join_drain(ampli_ctx *ctx)
{
    if (ctx->drain_pending) {
        HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_drain_done, 0));
        ctx->drain_pending = false;
    }
    return AMPLI_OK;
}

extern "C" int ampli_set_async_drain(ampli_ctx *ctx, int32_t on)
{
    if (!ctx) return AMPLI_E_INVALID;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (on && !ctx->side) {
        HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->side, hipStreamNonBlocking));
        HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_stream_done, hipEventDisableTiming));
        HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_drain_done, hipEventDisableTiming));
    }
    if (!on) { int rc = join_drain(ctx); if (rc) return rc; }
    ctx->async_drain = on ? 1 : 0;
    return AMPLI_OK;
}

extern "C" int ampli_wait_calls(ampli_ctx *ctx)
{
    if (!ctx) return AMPLI_E_INVALID;
    return join_drain(ctx);
}

// ---------------------------------------------------------------------------
// Position ranges on concurrent streams (ampli_set_ranges; include/amplisolve_hip.h).  With n > 1 ranges ampli_error_estimate and
// ampli_poisson_call (prefilter mode) cut the panel into n tile-aligned ranges of positions, every range on a stream the context
// created for it (lane_stream, ampli_internal.h), each range's poisson_call behind its own error_estimate.  The section opens with a fork (the
// lanes' streams wait for everything enqueued on the context's stream so far) and stays open across calls: back-to-back passes
// over independent batches overlap -- one range's poisson_call and another's error_reduce fill each other's partly filled rounds
// of workgroups.  It closes (the context's stream waits for every lane) at the next ordinary call: main_stream().
// ---------------------------------------------------------------------------
void range_cuts(const long long P, const int n, long long cut[AMPLI_MAX_RANGES + 1])
{
    const long long tiles = (P + 63) / 64;
    for (int k = 0; k < n; ++k) cut[k] = std::min<long long>(P, (tiles * k / n) * 64);
    cut[n] = P;
}

int ampli_ranges_join_internal(ampli_ctx *ctx)
{
    if (!ctx->ranges_open) return AMPLI_OK;
    // Every lane is joined whatever happens to another: a lane whose event cannot be recorded or waited for is waited for on the
    // host instead, and only a lane that cannot be joined at all leaves an error -- a sticky one (main_stream() has no way to return
    // it), which the entry point that asked for the stream reports from check_launch().  The section counts as closed only then.
    int rc = AMPLI_OK;
    for (int k = 0; k < ctx->n_ranges; ++k) {
        hipError_t e = hipEventRecord(ctx->lanes[k].done, ctx->lanes[k].stream);
        if (e == hipSuccess) e = hipStreamWaitEvent(ctx->stream, ctx->lanes[k].done, 0);
        if (e != hipSuccess) e = hipStreamSynchronize(ctx->lanes[k].stream);
        if (e != hipSuccess) {
            ctx->err = std::string("joining position range ") + std::to_string(k) + ": " + hipGetErrorString(e);
            ctx->sticky = rc = AMPLI_E_HIP;
        }
    }
    ctx->ranges_open = false;
    return rc;
}

// open the section for a panel of P positions (or keep it open if it is cut for the same panel)
int ranges_fork(ampli_ctx *ctx, const long long P)
{
    if (ctx->ranges_open && ctx->ranges_P == P) return AMPLI_OK;
    { int rc = ampli_ranges_join_internal(ctx); if (rc) return rc; }
    HIP_TRY(ctx, hipEventRecord(ctx->ev_fork, ctx->stream));
    for (int k = 0; k < ctx->n_ranges; ++k) HIP_TRY(ctx, hipStreamWaitEvent(ctx->lanes[k].stream, ctx->ev_fork, 0));
    ctx->ranges_open = true;
    ctx->ranges_P = P;
    return AMPLI_OK;
}

// ranges apply to a launch over P positions: switched on, not capturing, and every range at least two tiles
bool ranges_apply(ampli_ctx *ctx, const long long P)
{
    return ctx->n_ranges > 1 && (P + 63) / 64 >= 2ll * ctx->n_ranges && !is_capturing(ctx);
}

// Two streams overlap only if HIP has put them on different hardware queues -- it deals streams to a few queues (four by default) by
// rules of its own, and two ranges on one queue simply run one after the other (measured: three ranges of which two shared a queue,
// 0.18 ms per pass against 0.155 on one stream).  ampli_set_ranges therefore CHECKS: a short sleeping kernel on both streams at once
// takes its own time if they overlap and twice that if they do not; a stream that shares a queue with an earlier range's is
// replaced by a new one (a few tries).  ~0.2 ms per pair, once.
__global__ void lane_probe_kernel(const int iters)
{
    for (int i = 0; i < iters; ++i) __builtin_amdgcn_s_sleep(127); // 127 x 64 cycles: ~3.4 us per turn at 2.4 GHz; bounded
}

static int lanes_overlap(ampli_ctx *ctx, hipStream_t a, hipStream_t b, bool *overlap)
{
    struct Events { // destroyed on every path out
        hipEvent_t e[3] = {nullptr, nullptr, nullptr};
        ~Events() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
    } ev;
    for (hipEvent_t &x : ev.e) HIP_TRY(ctx, hipEventCreate(&x));
    hipEvent_t e0 = ev.e[0], e1 = ev.e[1], e2 = ev.e[2];
    float alone = 0, both = 0;
    for (int pass = 0; pass < 2; ++pass) { // the first pass warms the kernel's code object and both queues
        HIP_TRY(ctx, hipEventRecord(e0, a));
        hipLaunchKernelGGL(lane_probe_kernel, dim3(1), dim3(64), 0, a, 24);
        HIP_TRY(ctx, hipEventRecord(e1, a));
        HIP_TRY(ctx, hipStreamSynchronize(a));
        HIP_TRY(ctx, hipEventElapsedTime(&alone, e0, e1));
        HIP_TRY(ctx, hipEventRecord(e0, a));
        hipLaunchKernelGGL(lane_probe_kernel, dim3(1), dim3(64), 0, a, 24);
        hipLaunchKernelGGL(lane_probe_kernel, dim3(1), dim3(64), 0, b, 24);
        HIP_TRY(ctx, hipEventRecord(e1, a));
        HIP_TRY(ctx, hipEventRecord(e2, b));
        HIP_TRY(ctx, hipStreamSynchronize(a));
        HIP_TRY(ctx, hipStreamSynchronize(b));
        float ta = 0, tb = 0;
        HIP_TRY(ctx, hipEventElapsedTime(&ta, e0, e1));
        HIP_TRY(ctx, hipEventElapsedTime(&tb, e0, e2));
        both = ta > tb ? ta : tb;
    }
    *overlap = both < 1.6f * alone; // one after the other: ~2 x
    return check_launch(ctx, "lane_probe_kernel");
}

extern "C" int ampli_ranges_concurrent(const ampli_ctx *ctx) { return ctx ? ctx->ranges_verified : AMPLI_E_INVALID; }

extern "C" int ampli_set_ranges(ampli_ctx *ctx, int32_t n_ranges)
{
    if (!ctx) return AMPLI_E_INVALID;
    if (n_ranges < 1 || n_ranges > AMPLI_MAX_RANGES) return fail(ctx, AMPLI_E_INVALID, "set_ranges: 1 .. 4 ranges");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    { int rc = ampli_ranges_join_internal(ctx); if (rc) return rc; }
    if (n_ranges > 1 && !ctx->ev_fork) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming));
    ctx->ranges_verified = n_ranges > 1 ? 1 : 0;
    for (int k = 0; k < n_ranges && n_ranges > 1; ++k) {
        AmpliLane &l = ctx->lanes[k];
        if (!l.done) HIP_TRY(ctx, hipEventCreateWithFlags(&l.done, hipEventDisableTiming));
        if (l.stream && l.verified) continue; // kept from an earlier call: already known to overlap with the lanes before it
        struct Spare { // streams set aside during the search, destroyed on every path out
            hipStream_t s[8];
            int n = 0;
            ~Spare() { for (int i = 0; i < n; ++i) (void)hipStreamDestroy(s[i]); }
        } spare;
        bool ok = false;
        for (int attempt = 0; attempt < 8 && !ok; ++attempt) {
            if (!l.stream) HIP_TRY(ctx, hipStreamCreateWithFlags(&l.stream, hipStreamNonBlocking));
            ok = true;
            for (int j = 0; j < k && ok; ++j) {
                int rc = lanes_overlap(ctx, ctx->lanes[j].stream, l.stream, &ok);
                if (rc) return rc;
            }
            // a stream that shares a queue with an earlier range's is kept alive until the search ends: destroyed at once, the next one
            // created would take its place on the same queue
            if (!ok) { spare.s[spare.n++] = l.stream; l.stream = nullptr; }
        }
        if (!ok) { l.stream = spare.s[--spare.n]; ctx->ranges_verified = 0; } // no luck: the ranges still give the right results, two of them in turn
        l.verified = ok;
    }
    ctx->n_ranges = n_ranges;
    return AMPLI_OK;
}

extern "C" int ampli_ranges_join(ampli_ctx *ctx)
{
    if (!ctx) return AMPLI_E_INVALID;
    return ampli_ranges_join_internal(ctx);
}

// an event on range `range`'s stream, WITHOUT closing the section: brackets that range's share of the calls around it (the
// kernels' durations under the overlap the ranges exist for)
extern "C" int ampli_range_event_record(ampli_ctx *ctx, int32_t range, void *ev)
{
    if (!ctx || !ev || range < 0 || range >= ctx->n_ranges) return AMPLI_E_INVALID;
    // without ranges (n_ranges = 1) there are no lanes: range 0 is the context's own stream
    HIP_TRY(ctx, hipEventRecord((hipEvent_t)ev, ctx->n_ranges > 1 ? lane_stream(ctx, range) : main_stream(ctx)));
    return AMPLI_OK;
}

// ---------------------------------------------------------------------------
// hipGraph capture of a sequence of ampli_* calls (launch-bound small panels: a pass over a 10k-position panel is
// four ~10 us kernels, so the launches themselves dominate).  Capture needs a real stream (AMPLI_STREAM_OWN or any
// non-null stream) and warm workspaces: run the sequence once before capturing; a call that would have to allocate
// or synchronise while capturing fails with AMPLI_E_INVALID.
// ---------------------------------------------------------------------------
bool is_capturing(ampli_ctx *ctx)
{
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (!ctx->stream) return false;
    if (hipStreamIsCapturing(ctx->stream, &st) != hipSuccess) return false;
    return st == hipStreamCaptureStatusActive;
}

extern "C" int ampli_graph_begin(ampli_ctx *ctx)
{
    if (!ctx) return AMPLI_E_INVALID;
    if (!main_stream(ctx)) return fail(ctx, AMPLI_E_INVALID, "graph capture needs a non-default stream (AMPLI_STREAM_OWN)");
    { int rc = join_drain(ctx); if (rc) return rc; }
    HIP_TRY(ctx, hipStreamBeginCapture(main_stream(ctx), hipStreamCaptureModeThreadLocal));
    return AMPLI_OK;
}

extern "C" int ampli_graph_end(ampli_ctx *ctx, void **graph_exec)
{
    if (!ctx || !graph_exec) return AMPLI_E_INVALID;
    hipGraph_t g = nullptr;
    HIP_TRY(ctx, hipStreamEndCapture(main_stream(ctx), &g));
    hipGraphExec_t e = nullptr;
    hipError_t err = hipGraphInstantiate(&e, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    if (err != hipSuccess) return fail(ctx, AMPLI_E_HIP, "hipGraphInstantiate failed");
    *graph_exec = (void *)e;
    return AMPLI_OK;
}

extern "C" int ampli_graph_launch(ampli_ctx *ctx, void *graph_exec)
{
    if (!ctx || !graph_exec) return AMPLI_E_INVALID;
    HIP_TRY(ctx, hipGraphLaunch((hipGraphExec_t)graph_exec, main_stream(ctx)));
    return AMPLI_OK;
}

extern "C" int ampli_graph_destroy(void *graph_exec)
{
    return hipGraphExecDestroy((hipGraphExec_t)graph_exec) == hipSuccess ? AMPLI_OK : AMPLI_E_HIP;
}

extern "C" int ampli_sync(ampli_ctx *ctx)
{
    if (!ctx) return AMPLI_E_INVALID;
    { int rc = join_drain(ctx); if (rc) return rc; }
    HIP_TRY(ctx, hipStreamSynchronize(main_stream(ctx)));
    return AMPLI_OK;
}

extern "C" int ampli_pinned_alloc(size_t bytes, void **out)
{
    if (!out) return AMPLI_E_INVALID;
    return hipHostMalloc(out, bytes, hipHostMallocDefault) == hipSuccess ? AMPLI_OK : AMPLI_E_NOMEM;
}
extern "C" int ampli_pinned_free(void *p) { return hipHostFree(p) == hipSuccess ? AMPLI_OK : AMPLI_E_HIP; }
// pin memory the caller already owns and has filled (the command lines' parsers start before the runtime is up)
extern "C" int ampli_host_register(ampli_ctx *ctx, void *p, size_t bytes)
{
    if (!p || !bytes) return AMPLI_E_INVALID;
    if (ctx && hipSetDevice(ctx->device) != hipSuccess) return AMPLI_E_HIP; // the calling thread may not be the one that made the context
    return hipHostRegister(p, bytes, hipHostRegisterDefault) == hipSuccess ? AMPLI_OK : AMPLI_E_NOMEM;
}
extern "C" int ampli_host_unregister(void *p) { return hipHostUnregister(p) == hipSuccess ? AMPLI_OK : AMPLI_E_HIP; }

extern "C" int ampli_dev_alloc(ampli_ctx *ctx, size_t bytes, void **d_out)
{
    if (!ctx || !d_out) return AMPLI_E_INVALID;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (hipMalloc(d_out, bytes ? bytes : 1) != hipSuccess) return fail(ctx, AMPLI_E_NOMEM, "hipMalloc failed");
    return AMPLI_OK;
}
extern "C" int ampli_dev_free(ampli_ctx *ctx, void *d_p)
{
    if (!ctx) return AMPLI_E_INVALID;
    HIP_TRY(ctx, hipFree(d_p));
    return AMPLI_OK;
}
extern "C" int ampli_copy_h2d(ampli_ctx *ctx, void *d_dst, const void *src, size_t bytes)
{
    if (!ctx) return AMPLI_E_INVALID;
    HIP_TRY(ctx, hipMemcpyAsync(d_dst, src, bytes, hipMemcpyHostToDevice, main_stream(ctx)));
    return AMPLI_OK;
}
extern "C" int ampli_copy_d2h(ampli_ctx *ctx, void *dst, const void *d_src, size_t bytes)
{
    if (!ctx) return AMPLI_E_INVALID;
    { int rc = join_drain(ctx); if (rc) return rc; }
    HIP_TRY(ctx, hipMemcpyAsync(dst, d_src, bytes, hipMemcpyDeviceToHost, main_stream(ctx)));
    return AMPLI_OK;
}
extern "C" int ampli_memset_d(ampli_ctx *ctx, void *d_dst, int byte, size_t bytes)
{
    if (!ctx) return AMPLI_E_INVALID;
    HIP_TRY(ctx, hipMemsetAsync(d_dst, byte, bytes, main_stream(ctx)));
    return AMPLI_OK;
}

extern "C" int ampli_event_create(void **ev)
{
    if (!ev) return AMPLI_E_INVALID;
    hipEvent_t e;
    if (hipEventCreate(&e) != hipSuccess) return AMPLI_E_HIP;
    *ev = (void *)e;
    return AMPLI_OK;
}
extern "C" int ampli_event_destroy(void *ev) { return hipEventDestroy((hipEvent_t)ev) == hipSuccess ? AMPLI_OK : AMPLI_E_HIP; }
extern "C" int ampli_event_record(ampli_ctx *ctx, void *ev)
{
    if (!ctx) return AMPLI_E_INVALID;
    HIP_TRY(ctx, hipEventRecord((hipEvent_t)ev, main_stream(ctx)));
    return AMPLI_OK;
}
extern "C" int ampli_event_sync(void *ev) { return hipEventSynchronize((hipEvent_t)ev) == hipSuccess ? AMPLI_OK : AMPLI_E_HIP; }
extern "C" int ampli_event_elapsed_ms(void *a, void *b, float *ms)
{
    if (hipEventSynchronize((hipEvent_t)b) != hipSuccess) return AMPLI_E_HIP;
    return hipEventElapsedTime(ms, (hipEvent_t)a, (hipEvent_t)b) == hipSuccess ? AMPLI_OK : AMPLI_E_HIP;
}

extern "C" int ampli_set_record_layout(ampli_ctx *ctx, int32_t layout)
{
    if (!ctx) return AMPLI_E_INVALID;
    if (layout != AMPLI_RECORDS_I32 && layout != AMPLI_RECORDS_U16 && layout != AMPLI_RECORDS_U24)
        return fail(ctx, AMPLI_E_INVALID, "set_record_layout: unknown layout");
    ctx->rec_layout = layout;
    return AMPLI_OK;
}

extern "C" int ampli_set_slice_group(ampli_ctx *ctx, int32_t group_size, int32_t group_index)
{
    if (!ctx) return AMPLI_E_INVALID;
    if (group_size < 1 || group_index < 0 || group_index >= group_size) return fail(ctx, AMPLI_E_INVALID, "set_slice_group: 0 <= index < size");
    ctx->grp_size = group_size;
    ctx->grp_index = group_index;
    return AMPLI_OK;
}

extern "C" int ampli_set_tuning(ampli_ctx *ctx, int32_t reduce_sample_splits, int32_t reduce_general, int32_t reduce_lane_groups)
{
    if (!ctx || reduce_sample_splits < 0 || (reduce_lane_groups != 0 && reduce_lane_groups != 1 && reduce_lane_groups != 2 && reduce_lane_groups != 4))
        return AMPLI_E_INVALID;
    ctx->reduce_splits = reduce_sample_splits;
    ctx->reduce_general = reduce_general ? 1 : 0;
    ctx->reduce_groups = reduce_lane_groups; // lane groups per wave (0 = auto)
    return AMPLI_OK;
}

extern "C" int ampli_set_reduce_compact(ampli_ctx *ctx, int32_t on)
{
    if (!ctx) return AMPLI_E_INVALID;
    ctx->reduce_compact = on ? 1 : 0;
    ctx->reduce_compact_u16_only = on == 2 ? 1 : 0; // 2: the compact-state kernel for uint16 records only (A/B runs of the 24-bit form)
    return AMPLI_OK;
}

extern "C" int ampli_last_reduce_kernel(const ampli_ctx *ctx)
{
    return ctx && ctx->last_reduce_kernel >= 0 ? ctx->last_reduce_kernel : AMPLI_E_INVALID;
}

extern "C" int ampli_set_poisson_tuning(ampli_ctx *ctx, int32_t rows_per_wave, int32_t drain_blocks_per_shard)
{
    if (!ctx || rows_per_wave < 0 || drain_blocks_per_shard < 0 || drain_blocks_per_shard > 65535) return AMPLI_E_INVALID;
    ctx->pc_rows_per_wave = rows_per_wave;
    ctx->pc_drain_blocks = drain_blocks_per_shard;
    return AMPLI_OK;
}

extern "C" int ampli_set_queue_items(ampli_ctx *ctx, int64_t items)
{
    if (!ctx || items < 0) return AMPLI_E_INVALID;
    ctx->queue_min_items = (size_t)items;
    return AMPLI_OK;
}

extern "C" int ampli_mem_info(ampli_ctx *ctx, size_t *free_bytes, size_t *total_bytes)
{
    if (!ctx || !free_bytes || !total_bytes) return AMPLI_E_INVALID;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemGetInfo(free_bytes, total_bytes));
    return AMPLI_OK;
}

extern "C" int ampli_ctx_flags(ampli_ctx *ctx, int32_t *out, int32_t clear)
{
    if (!ctx || !out) return AMPLI_E_INVALID;
    { int rc = join_drain(ctx); if (rc) return rc; }
    HIP_TRY(ctx, hipMemcpyAsync(out, ctx->d_flags, sizeof(int), hipMemcpyDeviceToHost, main_stream(ctx)));
    HIP_TRY(ctx, hipStreamSynchronize(main_stream(ctx)));
    if (clear) HIP_TRY(ctx, hipMemsetAsync(ctx->d_flags, 0, sizeof(int), main_stream(ctx)));
    return AMPLI_OK;
}
