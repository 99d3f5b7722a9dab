// rt_api_frame.cpp — frames: rt_render_frame issues what the frame ring plans
// (rt_frame_ring.h) on one HIP stream per slot (the reference's MTL4CommandQueue + events,
// Renderer.swift:1405-1503); the per-frame statistics; and what reads a finished frame: rt_wait,
// the target reads, tile pack / unpack and rt_present.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "rt_ctx.h"

using namespace rt;

namespace {
// Default slots: eight when the HIP runtime gives the process at least eight hardware
// queues (GPU_MAX_HW_QUEUES, read once; HIP's default is 4), so every slot's stream has a queue of
// its own; four otherwise (more streams than queues serialise unrelated frames: eight slots on
// four queues measured 2.85 against 3.54 Grays/s per rank).  8-way rank share of C3g, eight
// queues: 4 slots 3.54 / 3.52, 8 slots 3.71 / 3.69; 4-way 4.73 / 4.70 -> 4.76 / 4.86.
int small_frame_slots() {
    static const int n = [] {
        const char* e = getenv("GPU_MAX_HW_QUEUES");
        return (e && atoi(e) >= 8) ? 8 : 4;
    }();
    return n;
}

hipStream_t slot_stream(rt_ctx* c, int k) { return k == 0 ? c->stream : (hipStream_t)c->slot[k].own_stream; }

// A tile set with its defaults (64-pixel tiles, one rank) over a w x h image: tiles per row and
// the tiles the rank owns (tile ids rank, rank + nranks, ...).
struct TileSet {
    int ts, rank, nranks, tiles_x, own;
};
TileSet resolve_tiles(int w, int h, const rt_tile_set* t) {
    TileSet s;
    s.ts = (t && t->tile_size > 0) ? t->tile_size : 64;
    s.nranks = (t && t->nranks > 0) ? t->nranks : 1;
    s.rank = (t && t->nranks > 0) ? t->rank : 0;
    s.tiles_x = (w + s.ts - 1) / s.ts;
    const int total = s.tiles_x * ((h + s.ts - 1) / s.ts);
    s.own = s.rank >= total ? 0 : (total - s.rank + s.nranks - 1) / s.nranks;
    return s;
}
// ... of the context's targets, as the device kernels take it
rt_status device_tiles(rt_ctx* c, const rt_tile_set* t, TileSet& s) {
    s = resolve_tiles(c->width, c->height, t);
    if (s.ts % 16 != 0) FAIL(c, RT_ERR_INVALID_ARG, "tile_size must be a multiple of 16");
    if (s.rank < 0 || s.rank >= s.nranks) FAIL(c, RT_ERR_INVALID_ARG, "bad rank");
    return RT_OK;
}
// ... of a host image
rt_status host_tiles(int32_t w, int32_t h, const rt_tile_set* t, TileSet& s) {
    s = resolve_tiles(w, h, t);
    if (w <= 0 || h <= 0 || s.rank < 0 || s.rank >= s.nranks) FAIL((rt_ctx*)nullptr, RT_ERR_INVALID_ARG, "bad tile set");
    return RT_OK;
}

// The slot's wavefront memory for `own_px` pixels: queues and path state by the frame's size, and
// once per slot the counters, events and pinned blocks.  Fills fs.wf in.
rt_status ensure_wavefront(rt_ctx* c, FrameSlot& fs, size_t own_px, int spp, int max_extra) {
    WavefrontBuffers& W = fs.wf;
    size_t paths = own_px * (size_t)(spp + max_extra);
    size_t npix = (size_t)c->width * c->height;
    if (paths >= (1ull << 32)) FAIL(c, RT_ERR_UNSUPPORTED, "too many paths for one frame");
    rt_status st;
    if (W.cap_paths < paths || W.queue_entries < wavefront_queue_entries(paths, max_extra)) {
        size_t qe = wavefront_queue_entries(paths, max_extra);
        if ((st = dev_alloc(c, fs.qc, 2 * qe * 16))) return st;   // both queues' colour arrays
        if ((st = dev_alloc(c, fs.qr, 2 * qe * 4))) return st;    // ... root-word arrays
        if ((st = dev_alloc(c, fs.accum, paths * 16))) return st;
        if ((st = dev_alloc(c, fs.meta, paths * 16))) return st;
        if ((st = dev_alloc(c, fs.q0, qe * 32))) return st;
        if ((st = dev_alloc(c, fs.q1, qe * 32))) return st;
        if ((st = dev_alloc(c, fs.hits, qe * 16))) return st;
        if ((st = dev_alloc(c, fs.sq, qe * 48))) return st;
        // hit sort output (4 float4 per hit), only with the sort on
        if (c->sort_bins && (st = dev_alloc(c, fs.sorted, qe * 64))) return st;
        W.cap_paths = paths;
        W.queue_entries = qe;
    }
    if (W.cap_pixels < npix || W.cap_pixels < own_px) {
        size_t px = std::max(npix, own_px);
        if ((st = dev_alloc(c, fs.extra, px * 8))) return st;
        W.cap_pixels = px;
    }
    if (c->sort_bins && !fs.sort_table.p) {
        if ((st = dev_alloc(c, fs.sort_table, (size_t)kSortMaxBins * kSortBlocks * 4))) return st;
        if ((st = dev_alloc(c, fs.sort_total, (size_t)kSortMaxBins * 4))) return st;
    }
    if (!fs.h_params) {   // the last one made below: a call that failed half way starts over
        if ((st = dev_alloc(c, fs.counts, kWfCountAllocBytes))) return st;
        HIPC(c, fs.h_counts.alloc(kWfCountAllocBytes));
        for (auto& e : fs.wf_ev) HIPC(c, e.create());
        for (auto& e : fs.tl_ev) HIPC(c, e.create());
        for (auto& e : fs.param_ev) HIPC(c, e.create());
        if ((st = dev_alloc(c, fs.params, sizeof(FrameParams)))) return st;
        HIPC(c, fs.h_params.alloc(sizeof(FrameParams) * WavefrontBuffers::kParamSlots));
        W.h_counts = fs.h_counts.get();
        std::copy(std::begin(fs.wf_ev), std::end(fs.wf_ev), W.ev);
        std::copy(std::begin(fs.tl_ev), std::end(fs.tl_ev), fs.wft.ev);
        std::copy(std::begin(fs.param_ev), std::end(fs.param_ev), W.param_ev);
        W.h_params = fs.h_params.get();
        W.d_params = (FrameParams*)fs.params.p;
    }
    W.qc[0] = (float4*)fs.qc.p;
    W.qc[1] = (float4*)fs.qc.p + W.queue_entries;
    W.qr[0] = (uint32_t*)fs.qr.p;
    W.qr[1] = (uint32_t*)fs.qr.p + W.queue_entries;
    W.p_accum = (float4*)fs.accum.p;
    W.p_meta = (uint4*)fs.meta.p;
    W.q[0] = (float4*)fs.q0.p;
    W.q[1] = (float4*)fs.q1.p;
    W.hits = (float4*)fs.hits.p;
    W.sq = (float4*)fs.sq.p;
    W.counts = (uint32_t*)fs.counts.p;
    W.tstamp = (unsigned long long*)((char*)fs.counts.p + kWfTsOffset);
    W.h_tstamp = (unsigned long long*)((char*)W.h_counts + kWfTsOffset);
    W.px_extra = (uint2*)fs.extra.p;
    W.sorted = (float4*)fs.sorted.p;
    W.sort_table = (uint32_t*)fs.sort_table.p;
    W.sort_total = (uint32_t*)fs.sort_total.p;
    return RT_OK;
}

// Folds a finished frame of slot k into rt_stats: its per-frame fields and the running totals.
// Waits for that frame: called before the slot is reused and from rt_wait, oldest frame first.
rt_status harvest(rt_ctx* c, int k) {
    FrameSlot& f = c->slot[k];
    if (!f.pending) return RT_OK;
    f.pending = false;
    HIPC(c, hipEventSynchronize(f.done));
    float ms = 0.0f;
    HIPC(c, hipEventElapsedTime(&ms, f.ev0, f.ev1));
    if (f.wavefront) {
        const char* err = nullptr;
        if (!wavefront_collect(f.wf, f.wft, &f.wfs, &err))
            FAIL(c, RT_ERR_HIP, std::string("wavefront stats: ") + (err ? err : "?"));
    }
    const WfFrameStats& w = f.wfs;   // all zero for a megakernel frame
    rt_stats& S = c->stats;
    S.last_frame_ms = ms;
    std::memcpy(S.kernel_ms, w.stage_ms, sizeof S.kernel_ms);
    if (!f.wavefront) S.kernel_ms[0] = ms;
    S.pipeline = f.wavefront ? RT_PIPELINE_WAVEFRONT : RT_PIPELINE_MEGAKERNEL;
    S.iterations = w.iterations;
    const unsigned long long* hc = f.h_counters.get();
    auto total = [hc](int word) {
        unsigned long long t = 0;
        for (int r = 0; r < kCntReplicas; ++r) t += hc[cnt_word(word, r)];
        return t;
    };
    // rays a producer retired on root mask 0 count as traced: the misses wf_trace would have resolved
    S.root_retired_rays = f.wavefront ? total(kCntRootRetired) : 0;
    // shadow rays a shading step resolved itself; those of wf_shade count as traced, where connect
    // would have counted them
    S.dark_shadow_rays = total(kCntDarkShadow);
    S.root_unoccluded_shadow_rays = f.wavefront ? total(kCntRootUnoccluded) : 0;
    S.trace_rays = w.trace_rays + S.root_retired_rays + (f.wavefront ? total(kCntShadeSkipped) : 0);
    S.trace_launches = w.trace_launches;
    S.trace_ms = w.trace_ms;
    S.trace_dev_ms = w.trace_dev_ms;
    S.trace_dev_launches = w.trace_dev_launches;
    S.finish_dev_ms = w.finish_dev_ms;
    S.finish_dev_launches = w.finish_dev_launches;
    S.trace_closest_rays = w.trace_closest_rays + S.root_retired_rays;
    S.finish_launches = w.finish_launches;
    S.closest_rays = total(kCntClosest);
    S.shadow_rays = total(kCntShadow);
    S.node_visits = total(kCntNodes);
    S.node_visits_lds = 0;
    S.tri_tests = total(kCntTris);
    S.paths = total(kCntPaths);
    S.trace_nodes = f.wavefront ? total(kCntTraceNodes) : 0;
    S.trace_tris = f.wavefront ? total(kCntTraceTris) : 0;
    S.trace_nodes_lds = 0;
    S.frames_total += 1;
    S.total_closest_rays += S.closest_rays;
    S.total_shadow_rays += S.shadow_rays;
    S.total_paths += S.paths;
    S.total_frame_ms += S.last_frame_ms;
    for (int i = 0; i < 7; ++i) S.total_kernel_ms[i] += S.kernel_ms[i];
    S.total_trace_rays += S.trace_rays;
    S.total_trace_closest_rays += S.trace_closest_rays;
    S.total_root_retired_rays += S.root_retired_rays;
    S.total_dark_shadow_rays += S.dark_shadow_rays;
    S.total_root_unoccluded_shadow_rays += S.root_unoccluded_shadow_rays;
    S.total_trace_ms += S.trace_ms;
    S.total_trace_launches += (uint64_t)S.trace_launches;
    S.total_trace_dev_ms += S.trace_dev_ms;
    S.total_trace_dev_launches += (uint64_t)S.trace_dev_launches;
    S.total_finish_dev_ms += S.finish_dev_ms;
    S.total_finish_dev_launches += (uint64_t)S.finish_dev_launches;
    S.total_finish_launches += (uint64_t)S.finish_launches;
    if (f.wavefront) {
        const int gm = w.graph_mode;   // host-driven frames (run_wavefront without a timeline) count as eager
        (gm == kGraphReplay ? S.total_graph_replays : gm == kGraphCapture ? S.total_graph_captures
         : gm == kGraphFallback ? S.total_graph_fallbacks : S.total_graph_eager) += 1;
    }
    if (total(kCntOverflow)) FAIL(c, RT_ERR_STATE, "traversal stack overflow");
    return RT_OK;
}

// The scene as the kernels take it, reading geometry generation `geo`.
DevScene device_scene(const rt_ctx* c, const Geo& geo) {
    DevScene S;
    std::memset(&S, 0, sizeof S);   // no stray padding bytes: the frame-graph key compares S byte for byte
    S.tris = (const float*)geo[Geo::tris].p;
    S.nodes8 = (const Bvh8Node*)geo[Geo::nodes].p;
    S.root_box = (const RootBoxes*)geo[Geo::root_box].p;
    S.tri_info = (const uint4*)c->d_tri_info.p;
    S.pos = (const float4*)geo[Geo::pos].p;
    S.prev_pos = (const float4*)geo[Geo::prev_pos].p;
    S.nrm = (const float4*)geo[Geo::nrm].p;
    S.tri_nrm = (const float4*)geo[Geo::tri_nrm].p;
    S.inst = (const float*)geo[Geo::inst].p;
    S.prev_inst = (const float*)geo[Geo::prev_inst].p;
    S.materials = (const Material*)c->d_mat.p;
    S.lights = (const Light*)c->d_lights.p;
    S.halton = (const HaltonDim*)c->d_halton.p;
    S.tri_bin = (const uint16_t*)geo[Geo::tri_bin].p;
    S.max_submeshes = c->max_sub;
    S.num_materials = (int)c->h_mat.size();
    S.num_tris = (int)c->num_tris;
    S.num_nodes8 = (int)geo.num_nodes8;
    S.textured = c->textured ? 1 : 0;
    if (c->textured) {
        S.tex_texels = (const uchar4*)c->d_tex_texels.p;
        S.tex_info = (const uint4*)c->d_tex_info.p;
        S.mat_tex = (const int4*)c->d_mat_tex.p;
        S.uv = (const float2*)c->d_uv.p;
        S.tex_lut = (const float*)c->d_tex_lut.p;
    }
    return S;
}

// The frame's parameter block: its targets as the plan rotates them, its tile set.  The
// wavefront-only targets (prim_hit, motion_prev) stay null.
FrameParams frame_params(const rt_ctx* c, const Uniforms* U, const FramePlan& pl, const FrameSlot& F, const TileSet& T) {
    FrameParams P;
    std::memset(&P, 0, sizeof P);
    P.U = *U;
    P.random = (const uint32_t*)c->d_random.p;
    P.accum_in = (const float4*)c->d_accum[c->ring.read_idx].p;
    P.accum_out = (float4*)c->d_accum[1 - c->ring.read_idx].p;
    P.depth = (float*)F.depth.p;
    P.motion = (float2*)c->d_motion[pl.motion_out].p;
    P.gbuffer = U->enableDenoiseGBuffer ? (float4*)F.gbuffer.p : nullptr;
    P.prim_hit = nullptr;
    P.motion_prev = nullptr;
    P.counters = (unsigned long long*)F.counters.p;
    P.tile_size = T.ts;
    P.rank = T.rank;
    P.nranks = T.nranks;
    P.tiles_x = T.tiles_x;
    return P;
}

// What the plan asks for before the frame's own work: the stream's waits, the generation flip,
// the drain and the new rotation of a changed number of frames in flight.
rt_status issue_plan(rt_ctx* c, const FramePlan& pl, hipStream_t stream) {
    const FrameSlot& prev = c->slot[pl.prev];
    if (pl.retile_wait) HIPC(c, hipStreamWaitEvent(stream, prev.done, 0));
    if (pl.ctx_wait) {
        HIPC(c, hipEventRecord(c->scene_ev, c->stream));
        HIPC(c, hipStreamWaitEvent(stream, c->scene_ev, 0));
    }
    if (pl.flip) {
        HIPC(c, hipEventRecord(c->uev, c->ustream));
        c->uev_valid = true;
    }
    if (pl.drain)
        if (rt_status st = drain_frames(c)) return st;
    if (pl.regen) {
        if (rt_status st = drain_queries(c)) return st;   // a pending ray query may read a generation freed here
        for (int g = pl.ngens; g < kGens; ++g)
            for (DevBuf& b : c->geo[g].buf) dev_free(c, b);
    }
    c->ring.begin_frame(pl);
    if (c->uev_valid) HIPC(c, hipStreamWaitEvent(stream, c->uev, 0));
    return RT_OK;
}

// Pack / unpack run on `stream` after the newest frame, without a host wait, and extend that
// frame's `done` event over themselves: the frame that next writes the same accumulation target
// (two frames later) waits for it before its resolve, so the gather of frame f overlaps the
// rendering of frame f+1.
// own_stream: the ctx stream (rt_pack_tiles / rt_unpack_tiles); otherwise `stream` as the caller gave it,
// the null stream included (a collective ordered on PyTorch's default stream must see the pack)
rt_status tiles_op(rt_ctx* c, const rt_tile_set* t, const void* src, void* dst, hipStream_t stream, bool pack,
                   bool own_stream) {
    if (!c || (pack ? !dst : !src)) FAIL(c, RT_ERR_INVALID_ARG, "null argument");
    if (!c->width) FAIL(c, RT_ERR_STATE, "no targets");
    TileSet T;
    rt_status st = device_tiles(c, t, T);
    if (st) return st;
    HIPC(c, hipSetDevice(c->device));
    if (own_stream) stream = c->stream;
    FrameSlot& f = c->slot[c->ring.last_slot];
    const bool after_frame = c->ring.newest_used();
    if (after_frame) HIPC(c, hipStreamWaitEvent(stream, f.done, 0));
    float4* accum = (float4*)c->d_accum[c->ring.read_idx].p;
    if (pack)
        launch_pack_tiles(accum, (float4*)dst, c->width, c->height, T.ts, T.rank, T.nranks, T.tiles_x, T.own, stream);
    else
        launch_unpack_tiles((const float4*)src, accum, c->width, c->height, T.ts, T.rank, T.nranks, T.tiles_x, T.own,
                            stream);
    HIPC(c, hipGetLastError());
    if (after_frame) HIPC(c, hipEventRecord(f.done, stream));
    c->ring.tiles_enqueued(own_stream);
    return RT_OK;
}
}  // namespace

// Waits for every frame in flight.  Everything that changes what frames read (scene, BVH,
// targets, transforms) runs after it, so a frame never sees a half-updated scene.
rt_status drain_frames(rt_ctx* c) {
    if (c->ustream) HIPC(c, hipStreamSynchronize(c->ustream));
    for (int k = 0; k < kMaxSlots; ++k)
        if (c->ring.slot[k].used) {
            HIPC(c, hipStreamSynchronize(slot_stream(c, k)));
            HIPC(c, hipEventSynchronize(c->slot[k].done));
        }
    return RT_OK;
}

extern "C" {

rt_status rt_resize(rt_ctx* c, int32_t w, int32_t h, const uint32_t* offsets) {
    if (!c || !offsets) FAIL(c, RT_ERR_INVALID_ARG, "null argument");
    if (rt_status dst = drain_frames(c)) return dst;
    if (w <= 0 || h <= 0 || (int64_t)w * h > (1ll << 30)) FAIL(c, RT_ERR_INVALID_ARG, "bad size");
    HIPC(c, hipSetDevice(c->device));
    size_t n = (size_t)w * h;
    rt_status st;
    if ((st = dev_upload(c, c->d_random, offsets, n * 4))) return st;
    for (int i = 0; i < 2; ++i) {
        if ((st = dev_alloc(c, c->d_accum[i], n * 16))) return st;
        HIPC(c, hipMemsetAsync(c->d_accum[i].p, 0, n * 16, c->stream));
        c->ring.ctx_work++;
    }
    for (DevBuf& m : c->d_motion) {
        if ((st = dev_alloc(c, m, n * 8))) return st;
        HIPC(c, hipMemsetAsync(m.p, 0, n * 8, c->stream));
    }
    for (FrameSlot& f : c->slot) {
        if ((st = dev_alloc(c, f.depth, n * 4))) return st;
        HIPC(c, hipMemsetAsync(f.depth.p, 0, n * 4, c->stream));
        dev_free(c, f.gbuffer);
        dev_free(c, f.prim_hit);
        f.pending = false;
    }
    c->ring.reset_targets();
    c->hist_valid = false;
    HIPC(c, hipStreamSynchronize(c->stream));
    c->width = w;
    c->height = h;
    c->last_moving = false;   // motion target cleared
    return RT_OK;
}

int32_t rt_tile_count(int32_t w, int32_t h, const rt_tile_set* t) { return resolve_tiles(w, h, t).own; }

// Plan (the frame ring), waits, parameters, launch, commit.
rt_status rt_render_frame(rt_ctx* c, const Uniforms* U, const rt_tile_set* tiles) {
    if (!c || !U) FAIL(c, RT_ERR_INVALID_ARG, "null argument");
    if (!c->bvh_ready) FAIL(c, RT_ERR_STATE, "rt_render_frame before rt_bvh_build");
    if (!c->width) FAIL(c, RT_ERR_STATE, "rt_render_frame before rt_resize");
    if (U->width != c->width || U->height != c->height) FAIL(c, RT_ERR_INVALID_ARG, "uniforms size != targets size");
    if (U->lightCount < 1 || U->lightCount > (int)c->h_lights.size()) FAIL(c, RT_ERR_INVALID_ARG, "bad lightCount");
    if (U->maxBounces > RT_MAX_BOUNCES) FAIL(c, RT_ERR_UNSUPPORTED, "maxBounces > 12 exceeds the Halton table");
    if (U->samplesPerPixel > 4096 || U->motionSamplingMaxExtraSamples > 4096) FAIL(c, RT_ERR_INVALID_ARG, "bad spp");
    HIPC(c, hipSetDevice(c->device));
    {   // a refit that degraded the tree past rt_tuning.refit_rebuild_pct: rebuild before this frame
        bool rebuilt = false;
        if (rt_status qst = check_refit_quality(c, &rebuilt)) return qst;
    }
    TileSet T;
    rt_status st = device_tiles(c, tiles, T);
    if (st) return st;
    size_t n = (size_t)c->width * c->height;
    // DebugTextureModeMotion reads sample 0's motion from later samples of the same pixel
    // (Raytracing.metal:483): only the per-pixel kernel orders samples that way.
    bool wavefront = c->pipeline == RT_PIPELINE_WAVEFRONT && U->debugTextureMode != DebugTextureModeMotion;
    // Frames in flight (Renderer.swift:1406-1409): wavefront frames on the context's own stream
    // rotate over the frames-in-flight slots; a caller's stream and the megakernel keep one.
    //  By default one slot per hardware queue the HIP runtime gives the process (four, eight with
    // GPU_MAX_HW_QUEUES >= 8), as many as fit in kSlotBudget, at least two: the finish tail's
    // latency-bound launch and the bulk rounds of the other frames fill each other's gaps (round 3,
    // C3g 1080p x 4 on one MI355X, 2 / 3 / 4 slots: 7.46-7.49 / 7.91-7.94 / 8.36-8.44 Grays/s;
    // 5 / 6 slots on four queues 7.23-7.28 / 7.59-7.67, 6 / 8 slots on eight queues 8.15-8.24 /
    // 8.34-8.37; configs[1] 720p, 3 / 4 slots: 5.95 / 7.38 in round 2)
    const int spp = std::max(U->samplesPerPixel, 1);
    const int max_extra = U->enableMotionAdaptiveSampling ? std::max(U->motionSamplingMaxExtraSamples, 0) : 0;
    int nfl = 1;
    if (wavefront && c->stream == c->own_stream)
        nfl = wf_in_flight((uint64_t)T.own * T.ts * T.ts * (uint64_t)(spp + max_extra), small_frame_slots(),
                           c->max_in_flight);
    const FramePlan pl = c->ring.plan_frame(nfl, wavefront, T.ts, T.rank, T.nranks);
    FrameSlot& F = c->slot[pl.slot];
    const FrameSlot& prev = c->slot[pl.prev];
    const hipStream_t stream = slot_stream(c, pl.slot);
    if ((st = harvest(c, pl.slot))) return st;   // the slot's previous frame (nfl back) has finished
    if ((st = issue_plan(c, pl, stream))) return st;
    if (U->enableDenoiseGBuffer && !F.gbuffer.p) {
        if ((st = dev_alloc(c, F.gbuffer, 4 * n * 16))) return st;
        HIPC(c, hipMemsetAsync(F.gbuffer.p, 0, 4 * n * 16, stream));
    }
    const DevScene S = device_scene(c, c->geo[pl.gen]);
    FrameParams P = frame_params(c, U, pl, F, T);
    if (wavefront) {
        if ((st = ensure_wavefront(c, F, (size_t)T.own * T.ts * T.ts, spp, max_extra))) return st;
        if ((st = dev_alloc(c, F.prim_hit, n * 16))) return st;
        P.prim_hit = (uint4*)F.prim_hit.p;
        P.motion_prev = (const float2*)c->d_motion[pl.motion_prev].p;
    }
    HIPC(c, hipMemsetAsync(F.counters.p, 0, sizeof(unsigned long long) * kCounterWords, stream));
    F.gbuf_written = U->enableDenoiseGBuffer != 0;
    // extra samples can only be non-zero when something moved in this frame or the previous one
    const bool moving = c->inst_moved || c->skin_moved ||
                        std::memcmp(&U->camera, &U->previousCamera, sizeof(Camera)) != 0;
    const bool extra_pass = moving || c->last_moving;
    c->last_moving = moving;
    HIPC(c, hipEventRecord(F.ev0, stream));
    F.wft.pending = false;
    F.wfs = WfFrameStats{};
    if (wavefront) {
        const char* err = nullptr;
        // finish threshold, grid shares and team drain by the frame's size and the frames in flight
        const WfSchedule sched = wf_schedule((uint32_t)T.own * (uint32_t)T.ts * (uint32_t)T.ts * (uint32_t)spp, nfl,
                                             c->tail_paths, c->tuning);
        if (T.own > 0 && !run_wavefront(S, P, F.wf, c->tuning, sched, T.own, c->counting, c->spans, c->sort_bins,
                                        extra_pass, stream, pl.cross ? (hipEvent_t)prev.done : nullptr, &F.wft, &F.wfs,
                                        &err, c->graphs))
            FAIL(c, RT_ERR_HIP, std::string("wavefront: ") + (err ? err : "?"));
        if (T.own == 0 && pl.cross) HIPC(c, hipStreamWaitEvent(stream, prev.done, 0));
    } else {
        if (pl.cross) HIPC(c, hipStreamWaitEvent(stream, prev.done, 0));
        int nblocks = T.own * (T.ts / 16) * (T.ts / 16);
        if (nblocks > 0) launch_megakernel(S, P, nblocks, c->counting, stream);
    }
    HIPC(c, hipGetLastError());
    HIPC(c, hipEventRecord(F.ev1, stream));
    HIPC(c, hipMemcpyAsync(F.h_counters, F.counters.p, sizeof(unsigned long long) * kCounterWords,
                           hipMemcpyDeviceToHost, stream));
    HIPC(c, hipEventRecord(F.done, stream));
    F.wavefront = wavefront;
    F.pending = true;
    c->ring.commit_frame(pl);
    c->stats.frames_in_flight = nfl;
    c->last_frame_index = U->frameIndex;
    return RT_OK;
}

rt_status rt_wait(rt_ctx* c) {
    if (!c) FAIL(c, RT_ERR_INVALID_ARG, "null ctx");
    HIPC(c, hipSetDevice(c->device));
    HIPC(c, hipStreamSynchronize(c->stream));
    int order[kMaxSlots];
    c->ring.harvest_order(order);
    for (int k : order)
        if (rt_status st = harvest(c, k)) return st;
    if (c->ring.newest_used()) HIPC(c, hipEventSynchronize(c->slot[c->ring.last_slot].done));   // and a pack / unpack after it
    if (rt_status st = drain_queries(c)) return st;   // ray queries, also those on a caller's stream
    if (c->q_overflow) {
        c->q_overflow = false;
        FAIL(c, RT_ERR_STATE, "traversal stack overflow in a ray query");
    }
    return RT_OK;
}

rt_status rt_read_radiance(rt_ctx* c, float* rgba) {
    if (!c || !rgba) FAIL(c, RT_ERR_INVALID_ARG, "null argument");
    if (!c->width) FAIL(c, RT_ERR_STATE, "no targets");
    rt_status st = rt_wait(c);
    if (st) return st;
    HIPC(c, hipMemcpy(rgba, c->d_accum[c->ring.read_idx].p, (size_t)c->width * c->height * 16, hipMemcpyDeviceToHost));
    return RT_OK;
}

rt_status rt_read_radiance_half(rt_ctx* c, uint16_t* rgba) {
    if (!c || !rgba) FAIL(c, RT_ERR_INVALID_ARG, "null argument");
    if (!c->width) FAIL(c, RT_ERR_STATE, "no targets");
    rt_status st = rt_wait(c);
    if (st) return st;
    const size_t n = (size_t)c->width * c->height;
    if ((st = dev_alloc(c, c->d_half, n * 8))) return st;
    launch_to_half((const float4*)c->d_accum[c->ring.read_idx].p, (ushort4*)c->d_half.p, n, c->stream);
    HIPC(c, hipGetLastError());
    HIPC(c, hipMemcpyAsync(rgba, c->d_half.p, n * 8, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    return RT_OK;
}

rt_status rt_read_aux(rt_ctx* c, float* depth, float* motion, float* gbuffer) {
    if (!c) FAIL(c, RT_ERR_INVALID_ARG, "null ctx");
    if (!c->width) FAIL(c, RT_ERR_STATE, "no targets");
    rt_status st = rt_wait(c);
    if (st) return st;
    size_t n = (size_t)c->width * c->height;
    const FrameSlot& f = c->slot[c->ring.last_slot];   // the newest frame's targets
    if (depth) HIPC(c, hipMemcpy(depth, f.depth.p, n * 4, hipMemcpyDeviceToHost));
    if (motion) HIPC(c, hipMemcpy(motion, c->d_motion[c->ring.motion_cur].p, n * 8, hipMemcpyDeviceToHost));
    if (gbuffer) {
        if (!f.gbuffer.p || !f.gbuf_written) FAIL(c, RT_ERR_STATE, "the newest frame wrote no G-buffer (enableDenoiseGBuffer off)");
        HIPC(c, hipMemcpy(gbuffer, f.gbuffer.p, 4 * n * 16, hipMemcpyDeviceToHost));
    }
    return RT_OK;
}

rt_status rt_present(rt_ctx* c, const rt_present_opts* o, uint8_t* host_rgba8) {
    if (!c || !host_rgba8) FAIL(c, RT_ERR_INVALID_ARG, "null argument");
    if (!c->width) FAIL(c, RT_ERR_STATE, "no targets");
    const int ow = (o && o->out_width > 0) ? o->out_width : c->width;
    const int oh = (o && o->out_height > 0) ? o->out_height : c->height;
    const int scaler = o ? o->scaler : RT_SCALER_NONE;
    const int encode = o ? o->encode : RT_ENCODE_SRGB8;
    const int passes = (o && o->denoise_passes > 0) ? o->denoise_passes : 3;
    if (scaler < RT_SCALER_NONE || scaler > RT_SCALER_DENOISED || (encode != RT_ENCODE_SRGB8 && encode != RT_ENCODE_LINEAR8))
        FAIL(c, RT_ERR_INVALID_ARG, "bad scaler / encode");
    if (scaler == RT_SCALER_DENOISED && passes > 6) FAIL(c, RT_ERR_INVALID_ARG, "denoise_passes > 6");
    if ((int64_t)ow * oh > (1ll << 28)) FAIL(c, RT_ERR_INVALID_ARG, "output too large");
    HIPC(c, hipSetDevice(c->device));
    rt_status st;
    const size_t n = (size_t)ow * oh;
    if (!c->d_present_thr.p) {   // linear value at which the sRGB code reaches k + 1 (k + 0.5 of 255)
        float thr[256];
        for (int k = 0; k < 255; ++k) {
            const double s = (k + 0.5) / 255.0;
            thr[k] = (float)(s <= 0.04045 ? s / 12.92 : std::pow((s + 0.055) / 1.055, 2.4));
        }
        thr[255] = INFINITY;
        if ((st = dev_upload(c, c->d_present_thr, thr, sizeof thr))) return st;
    }
    if ((st = dev_alloc(c, c->d_present_out, n * 4))) return st;
    const bool temporal = scaler == RT_SCALER_TEMPORAL || scaler == RT_SCALER_DENOISED;
    if (temporal && (c->hist_w != ow || c->hist_h != oh || !c->d_hist[0].p)) {
        for (int i = 0; i < 2; ++i) {
            if ((st = dev_alloc(c, c->d_hist[i], n * 16))) return st;
            if ((st = dev_alloc(c, c->d_hdepth[i], n * 4))) return st;
        }
        c->hist_w = ow;
        c->hist_h = oh;
        c->hist_valid = false;
    }
    // after the newest frame (and any pack / unpack of it)
    FrameSlot& f = c->slot[c->ring.last_slot];
    if (!c->ring.newest_used()) FAIL(c, RT_ERR_STATE, "rt_present before the first frame");
    const float4* color = (const float4*)c->d_accum[c->ring.read_idx].p;
    if (scaler == RT_SCALER_DENOISED) {   // render-size scratch: two ping-pong images, guide, albedo
        if (!f.gbuffer.p || !f.gbuf_written)
            FAIL(c, RT_ERR_STATE, "RT_SCALER_DENOISED needs the newest frame's G-buffer (enableDenoiseGBuffer)");
        const size_t rn = (size_t)c->width * c->height;
        if (c->den_n != rn || !c->d_den[0].p) {
            for (int i = 0; i < 4; ++i)
                if ((st = dev_alloc(c, c->d_den[i], rn * 16))) return st;
            c->den_n = rn;
        }
    }
    HIPC(c, hipStreamWaitEvent(c->stream, f.done, 0));
    if (scaler == RT_SCALER_DENOISED)
        color = launch_denoise(color, (const float*)f.depth.p, (const float4*)f.gbuffer.p, (float4*)c->d_den[0].p,
                               (float4*)c->d_den[1].p, (float4*)c->d_den[2].p, (float4*)c->d_den[3].p, c->width,
                               c->height, passes, c->stream);
    const int hi = c->hist_idx;
    launch_present(color, (const float*)f.depth.p,
                   (const float2*)c->d_motion[c->ring.motion_cur].p, temporal ? (const float4*)c->d_hist[hi].p : nullptr,
                   temporal ? (const float*)c->d_hdepth[hi].p : nullptr,
                   temporal ? (float4*)c->d_hist[1 - hi].p : nullptr, temporal ? (float*)c->d_hdepth[1 - hi].p : nullptr,
                   (uchar4*)c->d_present_out.p, (const float*)c->d_present_thr.p, c->width, c->height, ow, oh,
                   temporal ? RT_SCALER_TEMPORAL : scaler,
                   encode == RT_ENCODE_SRGB8 ? 1 : 0, (temporal && c->hist_valid && c->last_frame_index > 0) ? 1 : 0,
                   c->stream);
    HIPC(c, hipGetLastError());
    if (temporal) {
        c->hist_idx = 1 - hi;
        c->hist_valid = true;
    }
    HIPC(c, hipMemcpyAsync(host_rgba8, c->d_present_out.p, n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    return RT_OK;
}

rt_status rt_pack_tiles(rt_ctx* c, const rt_tile_set* t, void* dst) {
    return tiles_op(c, t, nullptr, dst, nullptr, true, true);
}

rt_status rt_unpack_tiles(rt_ctx* c, const rt_tile_set* t, const void* src) {
    return tiles_op(c, t, src, nullptr, nullptr, false, true);
}

rt_status rt_pack_tiles_on(rt_ctx* c, const rt_tile_set* t, void* dst, void* stream) {
    return tiles_op(c, t, nullptr, dst, (hipStream_t)stream, true, false);
}

rt_status rt_unpack_tiles_on(rt_ctx* c, const rt_tile_set* t, const void* src, void* stream) {
    return tiles_op(c, t, src, nullptr, (hipStream_t)stream, false, false);
}

rt_status rt_pack_tiles_host(int32_t w, int32_t h, const rt_tile_set* t, const float* src, float* dst) {
    if (!src || !dst) FAIL((rt_ctx*)nullptr, RT_ERR_INVALID_ARG, "null argument");
    TileSet T;
    rt_status st = host_tiles(w, h, t, T);
    if (st) return st;
    for (size_t i = 0; i < (size_t)T.ts * T.ts * T.own; ++i) {
        int x, y;
        tile_pixel(i, T.ts, T.rank, T.nranks, T.tiles_x, x, y);
        for (int q = 0; q < 4; ++q) dst[4 * i + q] = (x < w && y < h) ? src[4 * ((size_t)y * w + x) + q] : 0.0f;
    }
    return RT_OK;
}

rt_status rt_unpack_tiles_host(int32_t w, int32_t h, const rt_tile_set* t, const float* src, float* dst) {
    if (!src || !dst) FAIL((rt_ctx*)nullptr, RT_ERR_INVALID_ARG, "null argument");
    TileSet T;
    rt_status st = host_tiles(w, h, t, T);
    if (st) return st;
    for (size_t i = 0; i < (size_t)T.ts * T.ts * T.own; ++i) {
        int x, y;
        tile_pixel(i, T.ts, T.rank, T.nranks, T.tiles_x, x, y);
        if (x < w && y < h)
            for (int q = 0; q < 4; ++q) dst[4 * ((size_t)y * w + x) + q] = src[4 * i + q];
    }
    return RT_OK;
}

}  // extern "C"
