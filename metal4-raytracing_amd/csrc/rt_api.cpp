// rt_api.cpp — the context of the C ABI (include/rt_api.h): create / destroy, device memory,
// the setters, tuning and statistics.  Mirrors the responsibilities of the reference's Renderer
// (MetalRaytracing/Renderer.swift) for the hot path.  The scene, BVH and geometry updates are in
// rt_api_scene.cpp, frames and everything that reads them in rt_api_frame.cpp.
#include <algorithm>
#include <new>

#include "rt_ctx.h"

using namespace rt;

thread_local std::string rt_g_err;

namespace {
// rt_set_tuning bounds: a chunk grab past the end of a queue still adds the chunk size to its
// 32-bit counter, once per wave (at most ~16K waves resident); 4096 x 16K stays far below 2^32
// minus any queue the library allocates.  The shade grid is grid-stride, so more blocks than
// 64K buy nothing.
constexpr int kMaxTuneChunk = 4096;
constexpr int kMaxTuneShadeBlocks = 65536;
// rt_tuning.refit_rebuild_pct: 0 = the default, < 0 = never
constexpr int kRefitRebuildPctDefault = 150;

std::vector<HaltonDim> halton_table() {
    std::vector<HaltonDim> t(RT_HALTON_DIMS);
    halton_table_fill(t.data(), RT_HALTON_DIMS);
    return t;
}

// The streams, events and pinned blocks a context holds from the start.
hipError_t create_resources(rt_ctx* c) {
    hipError_t e = hipSetDevice(c->device);
    if (e == hipSuccess) e = c->own_stream.create();
    for (FrameSlot& f : c->slot) {
        if (e == hipSuccess) e = f.ev0.create();
        if (e == hipSuccess) e = f.ev1.create();
        if (e == hipSuccess) e = f.done.create(hipEventDisableTiming);
        if (e == hipSuccess) e = f.h_counters.alloc(sizeof(unsigned long long) * kCounterWords);
    }
    for (int k = 1; k < kMaxSlots; ++k)
        if (e == hipSuccess) e = c->slot[k].own_stream.create();
    if (e == hipSuccess) e = c->scene_ev.create(hipEventDisableTiming);
    if (e == hipSuccess) e = c->ustream.create();
    if (e == hipSuccess) e = c->uev.create(hipEventDisableTiming);
    return e;
}

// rt_tuning (0 = default) -> the kernels' resolved parameters
WfTuning resolve_tuning(const rt_tuning& t) {
    WfTuning w;
    if (t.trace_chunk > 0) w.chunk = t.trace_chunk;
    if (t.finish_chunk > 0) w.fchunk = t.finish_chunk;
    if (t.refill_min > 0) w.refill_min = t.refill_min;
    if (t.shade_min > 0) w.shade_min = t.shade_min;
    if (t.shade_min_drained != 0) w.shade_min_x = t.shade_min_drained;
    w.team = t.team == 0 ? -1 : t.team == 1 ? 0 : t.team;
    if (t.finish_grid_pct > 0) w.finish_frac = std::min(t.finish_grid_pct, 100);
    if (t.trace_grid_pct > 0) w.trace_frac = std::min(t.trace_grid_pct, 100);
    if (t.shade_blocks > 0) w.shade_blocks = (unsigned)std::max(8, t.shade_blocks) / 8u * 8u;
    w.host_ctl = t.host_rounds != 0;
    w.log = std::max(0, t.log);
    return w;
}
}  // namespace

rt_status dev_alloc(rt_ctx* c, DevBuf& b, size_t bytes) {
    HIPC(c, b.reserve(bytes, c->dev_bytes));
    return RT_OK;
}

rt_status dev_upload(rt_ctx* c, DevBuf& b, const void* src, size_t bytes, hipStream_t s) {
    rt_status st = dev_alloc(c, b, bytes);
    if (st) return st;
    if (bytes) HIPC(c, hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, s ? s : c->stream));
    if (bytes && !s) c->ring.ctx_work++;
    return RT_OK;
}

int refit_rebuild_pct(const rt_ctx* c) {
    const int p = c->tuning_req.refit_rebuild_pct;
    return p == 0 ? kRefitRebuildPctDefault : p;
}

extern "C" {

const char* rt_version(void) {
    return "rt_hip 0.4 (gfx950, SAH-DP compressed 8-wide BVH, PLOC device build, wavefront with frames in flight + megakernel, USD + PNG ingest, denoised present)";
}

const char* rt_last_error(const rt_ctx* ctx) { return ctx ? ctx->err.c_str() : rt_g_err.c_str(); }

rt_status rt_create(const rt_opts* opts, rt_ctx** out) {
    if (!out) FAIL((rt_ctx*)nullptr, RT_ERR_INVALID_ARG, "out is null");
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) FAIL((rt_ctx*)nullptr, RT_ERR_NO_DEVICE, "no HIP device");
    rt_ctx* c = new (std::nothrow) rt_ctx();
    if (!c) FAIL((rt_ctx*)nullptr, RT_ERR_OUT_OF_MEMORY, "alloc ctx");
    if (opts) {
        c->device = opts->device;
        c->pipeline = opts->pipeline;
        c->tail_paths = opts->tail_paths;
        c->sort_bins = opts->sort_bins == 0 ? kSortBinsDefault : std::max(opts->sort_bins, 0);
    }
    if (c->device < 0 || c->device >= ndev) { delete c; FAIL((rt_ctx*)nullptr, RT_ERR_INVALID_ARG, "bad device ordinal"); }
    if (c->pipeline != RT_PIPELINE_MEGAKERNEL && c->pipeline != RT_PIPELINE_WAVEFRONT) {
        delete c;
        FAIL((rt_ctx*)nullptr, RT_ERR_INVALID_ARG, "bad pipeline");
    }
    if (c->sort_bins && (c->sort_bins < kSortMinBins || c->sort_bins > kSortMaxBins ||
                         (c->sort_bins & (c->sort_bins - 1)))) {
        delete c;
        FAIL((rt_ctx*)nullptr, RT_ERR_INVALID_ARG, "sort_bins must be a power of two in [1024, 4096]");
    }
    if (opts && opts->frames_in_flight > 0) c->max_in_flight = std::min(opts->frames_in_flight, kMaxSlots);
    hipError_t e = create_resources(c);
    if (e != hipSuccess) {
        rt_g_err = std::string("HIP init: ") + hipGetErrorString(e);
        delete c;
        return RT_ERR_HIP;
    }
    c->stream = c->own_stream;
    auto tab = halton_table();
    rt_status st = dev_upload(c, c->d_halton, tab.data(), tab.size() * sizeof(HaltonDim));
    for (FrameSlot& f : c->slot)
        if (!st) st = dev_alloc(c, f.counters, sizeof(unsigned long long) * kCounterWords);

    if (!st && hipStreamSynchronize(c->stream) != hipSuccess) st = RT_ERR_HIP;
    if (st) {
        rt_g_err = c->err;
        rt_destroy(c);
        return st;
    }
    *out = c;
    return RT_OK;
}

// Everything the context holds is released by its owners (rt_resources.h) once nothing runs.
rt_status rt_destroy(rt_ctx* c) {
    if (!c) return RT_OK;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->ustream) (void)hipStreamSynchronize(c->ustream);
    for (FrameSlot& f : c->slot)
        if (f.own_stream) (void)hipStreamSynchronize(f.own_stream);
    for (QuerySlot& q : c->qslot)   // ray queries, also those on a caller's stream
        if (q.pending) (void)hipEventSynchronize(q.done);
    delete c;
    return RT_OK;
}

rt_status rt_set_stream(rt_ctx* c, void* s) {
    if (!c) FAIL(c, RT_ERR_INVALID_ARG, "null ctx");
    rt_status st = drain_frames(c);
    if (st) return st;
    c->stream = s ? (hipStream_t)s : (hipStream_t)c->own_stream;
    return RT_OK;
}

rt_status rt_set_counting(rt_ctx* c, int32_t enabled) {
    if (!c) FAIL(c, RT_ERR_INVALID_ARG, "null ctx");
    c->counting = enabled != 0;
    return RT_OK;
}

rt_status rt_set_device_spans(rt_ctx* c, int32_t enabled) {
    if (!c) FAIL(c, RT_ERR_INVALID_ARG, "null ctx");
    c->spans = enabled != 0;
    return RT_OK;
}

rt_status rt_set_tuning(rt_ctx* c, const rt_tuning* t) {
    if (!c) FAIL(c, RT_ERR_INVALID_ARG, "null context");
    rt_tuning v{};
    if (t) v = *t;
    if (v.team != 0 && v.team != 1 && v.team != 2 && v.team != 4 && v.team != 8)
        FAIL(c, RT_ERR_INVALID_ARG, "rt_tuning.team must be 0 (default), 1 (off), 2, 4 or 8");
    // chunk grabs are 32-bit atomicAdds of the chunk size by every wave of the grid (and base + chunk
    // is formed in 32 bits): bounded so that neither can wrap for any queue the library allocates
    if (v.trace_chunk < 0 || v.trace_chunk > kMaxTuneChunk || v.finish_chunk < 0 || v.finish_chunk > kMaxTuneChunk ||
        v.refill_min < 0 || v.refill_min > 64 || v.shade_min < 0 || v.shade_min > 64 || v.shade_min_drained > 64 ||
        v.shade_min_drained < -100 || v.finish_grid_pct < 0 || v.finish_grid_pct > 100 || v.trace_grid_pct < 0 ||
        v.trace_grid_pct > 100 || v.shade_blocks < 0 || v.shade_blocks > kMaxTuneShadeBlocks || v.log < 0 || v.log > 2 ||
        v.device_bvh < 0 || v.device_bvh > 1 || (v.refit_rebuild_pct > 0 && v.refit_rebuild_pct < 100))
        FAIL(c, RT_ERR_INVALID_ARG, "rt_tuning field out of range");
    // frames already in flight keep the parameters they were enqueued with (their graphs' keys)
    c->tuning_req = v;
    c->tuning = resolve_tuning(v);
    return RT_OK;
}

rt_status rt_get_tuning(const rt_ctx* c, rt_tuning* out) {
    if (!c || !out) FAIL((rt_ctx*)nullptr, RT_ERR_INVALID_ARG, "null argument");
    const WfTuning& w = c->tuning;
    rt_tuning t{};
    t.trace_chunk = w.chunk;
    t.finish_chunk = w.fchunk;
    t.refill_min = w.refill_min;
    t.shade_min = w.shade_min;
    t.shade_min_drained = w.shade_min_x;
    t.team = c->tuning_req.team;
    t.finish_grid_pct = w.finish_frac;
    t.trace_grid_pct = w.trace_frac;
    t.shade_blocks = (int32_t)w.shade_blocks;
    t.host_rounds = w.host_ctl ? 1 : 0;
    t.log = w.log;
    t.device_bvh = c->tuning_req.device_bvh;
    t.refit_rebuild_pct = refit_rebuild_pct(c);
    *out = t;
    return RT_OK;
}

rt_status rt_set_graphs(rt_ctx* c, int32_t enabled) {
    if (!c) FAIL(c, RT_ERR_INVALID_ARG, "null ctx");
    c->graphs = enabled != 0;
    return RT_OK;
}

// The last frame's fields and the running totals are kept in c->stats as frames finish (harvest,
// rt_api_frame.cpp) and the tree's figures as it is built and refitted (rt_api_scene.cpp).
rt_status rt_get_stats(rt_ctx* c, rt_stats* out) {
    if (!c || !out) FAIL(c, RT_ERR_INVALID_ARG, "null argument");
    rt_status st = rt_wait(c);
    if (st) return st;
    c->stats.bvh_nodes = c->num_nodes8;
    c->stats.triangles = c->num_tris;
    c->stats.device_bytes = c->dev_bytes;
    *out = c->stats;
    return RT_OK;
}

}  // extern "C"
