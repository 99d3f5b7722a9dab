// rt_api_query.cpp — device ray queries: rt_trace_closest / rt_trace_any enqueue one rq_trace
// launch (rt_query.hip) over the caller's device rays against the geometry generation the next
// frame would read, and rt_get_query_stats reports them.  The replacement of Metal's
// `intersector.intersect` called outside raytracingKernel.  rt_resolve_hits enqueues one
// rq_resolve launch that turns rays and their hit records into surface and material records, by
// the same generation rule, and rt_shade_hits one rq_shade launch that turns those records and the
// path states into the paths' next rays (lights and Halton table only).  The path queries
// (rt_camera_paths, rt_compact_paths, rt_connect_paths, rt_retire_paths, rt_average_samples) close
// that loop, each one slot and one launch (the compaction: three, on the slot's own scratch).
// Every entry point is its argument checks, then enqueue_query around the parameter fill and the
// launch.  The _indirect forms are the same functions with a Count that carries a device word: the
// host then uses its `n` as the direct forms do (checks, grid, scratch, early return) and never
// reads the word; the kernels clamp it to `n` (launch_count, rt_kernels.h).  Queries share nothing writable with frames: their counters, events and statistics are
// their own (QuerySlot, rt_ctx.h).
#include <algorithm>
#include <cstring>

#include "rt_paths.h"
#include "rt_scene_host.h"

using namespace rt;

namespace {
// Folds the finished query of slot k into rt_query_stats.  Waits for it: called before the slot
// is reused and from drain_queries, oldest query first.
rt_status harvest_query(rt_ctx* c, int k) {
    QuerySlot& q = c->qslot[k];
    if (!q.pending) return RT_OK;
    q.pending = false;
    HIPC(c, hipEventSynchronize(q.done));
    if (!q.counted) return RT_OK;   // waited for, not part of rt_query_stats
    float ms = 0.0f;
    HIPC(c, hipEventElapsedTime(&ms, q.ev0, q.ev1));
    const unsigned long long* hc = q.h_counters.get();
    auto total = [hc](int word) {
        unsigned long long t = 0;
        for (int r = 0; r < kCntReplicas; ++r) t += hc[cnt_word(word, r)];
        return t;
    };
    rt_query_stats& S = c->qstats;
    S.rays = total(q.any ? kCntShadow : kCntClosest);
    S.hits = total(kCntPaths);
    S.node_visits = total(kCntNodes);
    S.tri_tests = total(kCntTris);
    S.grid_blocks = q.blocks;
    S.any_hit = q.any ? 1 : 0;
    S.device_ms = ms;
    S.queries_total += 1;
    S.total_rays += S.rays;
    S.total_hits += S.hits;
    S.total_node_visits += S.node_visits;
    S.total_tri_tests += S.tri_tests;
    S.total_grid_blocks += S.grid_blocks;
    S.total_device_ms += ms;
    if (total(kCntOverflow)) c->q_overflow = true;
    return RT_OK;
}

// The slot's device state, pinned copy and events, made once.
rt_status ensure_query_slot(rt_ctx* c, QuerySlot& q) {
    if (q.done) return RT_OK;   // the last one made below: a call that failed half way starts over
    if (rt_status st = dev_alloc(c, q.state, kRqStateBytes)) return st;
    HIPC(c, q.h_counters.alloc(sizeof(unsigned long long) * kCounterWords));
    HIPC(c, q.ev0.create());
    HIPC(c, q.ev1.create());
    HIPC(c, q.done.create(hipEventDisableTiming));
    return RT_OK;
}

// Where a query runs: the context's stream (the plain entry points), or the stream the caller
// gave as it is, the null stream included (the _on entry points).
struct QueryStream {
    hipStream_t s;
    bool own;
    static QueryStream of_ctx() { return {nullptr, true}; }
    static QueryStream on(void* stream) { return {(hipStream_t)stream, false}; }
};

// What every query does before its launch: takes the oldest slot (its previous query, kQuerySlots
// back, has finished) and makes the stream wait for the geometry the next frame would read: the
// generation updates since the newest frame went into (after the update stream's work so far),
// else the one frames read (after the event of the flip that made it current).  Gives the stream,
// the slot and that generation.
rt_status begin_query(rt_ctx* c, QueryStream where, hipStream_t& stream, QuerySlot*& q, const Geo*& geo) {
    HIPC(c, hipSetDevice(c->device));
    stream = where.own ? c->stream : where.s;
    q = &c->qslot[c->qnext];
    rt_status st = harvest_query(c, c->qnext);
    if (!st) st = ensure_query_slot(c, *q);
    if (st) return st;
    if (c->ring.gdirty) {
        if (!c->q_uev) HIPC(c, c->q_uev.create(hipEventDisableTiming));
        HIPC(c, hipEventRecord(c->q_uev, c->ustream));
        HIPC(c, hipStreamWaitEvent(stream, c->q_uev, 0));
    } else if (c->uev_valid) {
        HIPC(c, hipStreamWaitEvent(stream, c->uev, 0));
    }
    geo = &c->geo[c->ring.write_gen()];
    return RT_OK;
}

// After the launch: `done` marks its end for updates, rt_wait and rt_destroy (drain_queries).
rt_status commit_query(rt_ctx* c, QuerySlot& q, hipStream_t stream, bool counted) {
    HIPC(c, hipEventRecord(q.done, stream));
    q.pending = true;
    q.counted = counted;
    c->qnext = (c->qnext + 1) % kQuerySlots;
    return RT_OK;
}

// One query around its launch: begin_query, then body(slot, geometry, stream), which fills the
// parameters and launches on that stream, then the launch's error and commit_query.  counted: the
// body took the slot's events and counters for rt_query_stats (the traces).
template <class Body>
rt_status enqueue_query(rt_ctx* c, QueryStream where, bool counted, Body body) {
    hipStream_t stream = nullptr;
    QuerySlot* q = nullptr;
    const Geo* geo = nullptr;
    if (rt_status st = begin_query(c, where, stream, q, geo)) return st;
    if (rt_status st = body(*q, *geo, stream)) return st;
    HIPC(c, hipGetLastError());
    return commit_query(c, *q, stream, counted);
}

// A query's record count: the host's n (the direct forms), or a device word bounded by n (the
// _indirect forms; dev is set exactly when n > 0 there).
struct Count {
    uint32_t n;
    const uint32_t* dev;
    Count(uint32_t n_, const uint32_t* dev_ = nullptr) : n(n_), dev(dev_) {}
};

// What every _indirect entry point checks before it calls its direct form's function with a Count.
template <class Call>
rt_status with_device_count(rt_ctx* c, const rt_device_count* cnt, Call call) {
    if (!c) FAIL(c, RT_ERR_INVALID_ARG, "null ctx");
    if (!cnt) FAIL(c, RT_ERR_INVALID_ARG, "null device count");
    if (cnt->max > 0 && !cnt->count) FAIL(c, RT_ERR_INVALID_ARG, "null count pointer with max > 0");
    if ((uintptr_t)cnt->count & 3u) FAIL(c, RT_ERR_INVALID_ARG, "the count pointer must be 4-byte aligned");
    return call(Count(cnt->max, cnt->max > 0 ? cnt->count : nullptr));
}

// a small batch does not launch the whole chip
unsigned query_grid(unsigned resident, uint32_t n) { return std::min(resident, (n - 1u) / (unsigned)kBlock + 1u); }

rt_status trace(rt_ctx* c, const rt_ray* rays, Count cnt, void* out, bool any, QueryStream where) {
    const uint32_t n = cnt.n;
    if (!c) FAIL(c, RT_ERR_INVALID_ARG, "null ctx");
    if (n > 0) {
        if (!rays || !out) FAIL(c, RT_ERR_INVALID_ARG, "null argument");
        if (((uintptr_t)rays & 15u) || ((uintptr_t)out & (any ? 3u : 15u)))
            FAIL(c, RT_ERR_INVALID_ARG, "rays / hits must be 16-byte aligned, occluded 4-byte aligned");
    }
    if (!c->bvh_ready) FAIL(c, RT_ERR_STATE, "ray query before rt_bvh_build");
    if (n == 0) return RT_OK;
    return enqueue_query(c, where, true, [&](QuerySlot& q, const Geo& geo, hipStream_t stream) -> rt_status {
        DevScene S;
        std::memset(&S, 0, sizeof S);   // the traversal reads the tree, the triangles and tri_info only
        S.tris = (const float*)geo[Geo::tris].p;
        S.nodes8 = (const Bvh8Node*)geo[Geo::nodes].p;
        S.tri_info = (const uint4*)c->d_tri_info.p;
        S.max_submeshes = c->max_sub;
        S.num_tris = (int)c->num_tris;
        S.num_nodes8 = (int)geo.num_nodes8;
        RqParams Q;
        Q.rays = (const float4*)rays;
        Q.hits = any ? nullptr : (float4*)out;
        Q.occluded = any ? (uint32_t*)out : nullptr;
        Q.sub_first = (const uint32_t*)c->d_sub_first.p;
        Q.state = (unsigned long long*)q.state.p;
        Q.count = cnt.dev;
        Q.n = n;
        Q.refill_min = c->tuning.refill_min;
        q.any = any;
        q.blocks = query_grid(query_resident_blocks(), n);
        HIPC(c, hipMemsetAsync(q.state.p, 0, kRqStateBytes, stream));
        HIPC(c, hipEventRecord(q.ev0, stream));
        launch_query(S, Q, any, c->counting, q.blocks, stream);
        HIPC(c, hipGetLastError());   // here too: before the calls below can replace it
        HIPC(c, hipEventRecord(q.ev1, stream));
        HIPC(c, hipMemcpyAsync(q.h_counters, q.state.p, sizeof(unsigned long long) * kCounterWords, hipMemcpyDeviceToHost,
                               stream));
        return RT_OK;
    });
}

rt_status resolve(rt_ctx* c, const rt_ray* rays, const rt_ray_hit* hits, Count cnt, rt_surface* surfaces,
                  rt_surface_material* materials, QueryStream where) {
    const uint32_t n = cnt.n;
    if (!c) FAIL(c, RT_ERR_INVALID_ARG, "null ctx");
    if (n > 0) {
        if (!rays || !hits || !surfaces) FAIL(c, RT_ERR_INVALID_ARG, "null argument");
        if (((uintptr_t)rays | (uintptr_t)hits | (uintptr_t)surfaces | (uintptr_t)materials) & 15u)
            FAIL(c, RT_ERR_INVALID_ARG, "rays, hits, surfaces and materials must be 16-byte aligned");
    }
    if (!c->bvh_ready) FAIL(c, RT_ERR_STATE, "surface query before rt_bvh_build");
    if (n == 0) return RT_OK;
    return enqueue_query(c, where, false, [&](QuerySlot&, const Geo& geo, hipStream_t stream) -> rt_status {
        DevScene S;
        std::memset(&S, 0, sizeof S);   // surface_eval reads the shading streams only, not the tree
        S.pos = (const float4*)geo[Geo::pos].p;
        S.tri_nrm = (const float4*)geo[Geo::tri_nrm].p;
        S.inst = (const float*)geo[Geo::inst].p;
        S.materials = (const Material*)c->d_mat.p;
        S.max_submeshes = c->max_sub;
        S.num_materials = (int)c->h_mat.size();
        S.num_tris = (int)c->num_tris;
        S.textured = c->textured ? 1 : 0;
        if (c->textured) {
            S.tex_texels = (const uchar4*)c->d_tex_texels.p;
            S.tex_info = (const uint4*)c->d_tex_info.p;
            S.mat_tex = (const int4*)c->d_mat_tex.p;
            S.uv = (const float2*)c->d_uv.p;
            S.tex_lut = (const float*)c->d_tex_lut.p;
        }
        RsParams P;
        P.rays = (const float4*)rays;
        P.hits = (const float4*)hits;
        P.surfaces = (float4*)surfaces;
        P.materials = (float4*)materials;
        P.count = cnt.dev;
        P.n = n;
        launch_resolve(S, P, query_grid(resolve_resident_blocks(), n), stream);
        return RT_OK;
    });
}

// From here on no query reads the geometry: shading reads the lights and the Halton table only.
rt_status shade(rt_ctx* c, const rt_shade_opts* o, const rt_ray* rays, const rt_surface* surfaces,
                const rt_surface_material* materials, const float* randoms, Count cnt, rt_path* paths, rt_ray* next_rays,
                rt_ray* shadow_rays, float* contrib, QueryStream where) {
    const uint32_t n = cnt.n;
    if (!c) FAIL(c, RT_ERR_INVALID_ARG, "null ctx");
    if (rt_status st = validate_shade(c, o, rays, surfaces, materials, randoms, n, paths, next_rays, shadow_rays, contrib))
        return st;
    if (!c->scene_ready) FAIL(c, RT_ERR_STATE, "shading query before rt_scene_upload");
    int lights = 0;
    if (rt_status st = shade_light_count(c, o, (uint32_t)c->h_lights.size(), lights)) return st;
    if (n == 0) return RT_OK;
    return enqueue_query(c, where, false, [&](QuerySlot&, const Geo&, hipStream_t stream) -> rt_status {
        ShParams P;
        P.rays = (const float4*)rays;
        P.surfaces = (const float4*)surfaces;
        P.materials = (const float4*)materials;
        P.randoms = (const float4*)randoms;
        P.paths = (float4*)paths;
        P.next_rays = (float4*)next_rays;
        P.shadow_rays = (float4*)shadow_rays;
        P.contrib = (float4*)contrib;
        P.lights = (const Light*)c->d_lights.p;
        P.halton = (const HaltonDim*)c->d_halton.p;
        P.count = cnt.dev;
        P.n = n;
        P.shading_mode = o->shading_mode;
        P.max_bounces = o->max_bounces;
        P.light_count = lights;
        launch_shade(P, query_grid(shade_resident_blocks(), n), stream);
        return RT_OK;
    });
}

rt_status camera_paths(rt_ctx* c, const Uniforms* u, const rt_camera_opts* o, const uint32_t* random, uint32_t n,
                       rt_ray* rays, rt_path* paths, QueryStream where) {
    if (!c) FAIL(c, RT_ERR_INVALID_ARG, "null ctx");
    if (rt_status st = validate_camera(c, u, o, random, n, rays, paths)) return st;
    if (!random) {
        if (!c->width) FAIL(c, RT_ERR_STATE, "rt_camera_paths without offsets before rt_resize");
        if (u->width != c->width || u->height != c->height)
            FAIL(c, RT_ERR_STATE, "uniforms size != the size of the context's offsets (rt_resize)");
        random = (const uint32_t*)c->d_random.p;
    }
    if (n == 0) return RT_OK;
    return enqueue_query(c, where, false, [&](QuerySlot&, const Geo&, hipStream_t stream) -> rt_status {
        CamParams P;
        P.U = *u;
        P.random = random;
        P.halton = (const HaltonDim*)c->d_halton.p;
        P.rays = (float4*)rays;
        P.paths = (float4*)paths;
        P.n = n;
        P.first_pixel = o->first_pixel;
        P.tag_stride = o->tag_stride;
        P.tag_offset = o->tag_offset;
        P.sample = o->sample;
        launch_camera(P, query_grid(path_resident_blocks(), n), stream);
        return RT_OK;
    });
}

rt_status compact_paths(rt_ctx* c, const rt_path* paths, Count cnt, uint32_t mask, const rt_compact_stream* streams,
                        uint32_t stream_count, uint32_t* index, uint32_t* count, QueryStream where) {
    const uint32_t n = cnt.n;
    if (!c) FAIL(c, RT_ERR_INVALID_ARG, "null ctx");
    if (rt_status st = validate_compact(c, paths, n, mask, streams, stream_count, index, count)) return st;
    // the copy launch reads the input count after the scan launch wrote the output
    if (cnt.dev && cnt.dev == count) FAIL(c, RT_ERR_INVALID_ARG, "count is the device count it is compacted by");
    if (n == 0) return RT_OK;
    return enqueue_query(c, where, false, [&](QuerySlot& q, const Geo&, hipStream_t stream) -> rt_status {
        // The slot's own storage: its previous query has been harvested, so nothing reads what a growth
        // frees.  Grown to the largest size any compaction asked for, so the slots stop growing together.
        const size_t need = compact_scratch_bytes(n);
        c->q_scratch_max = std::max(c->q_scratch_max, need);
        if (q.scratch.bytes < need)
            if (rt_status st = dev_alloc(c, q.scratch, c->q_scratch_max)) return st;
        CompactParams P;
        std::memset(&P, 0, sizeof P);
        P.paths = (const float4*)paths;
        for (uint32_t k = 0; k < stream_count; ++k) {
            P.src[k] = (const float4*)streams[k].src;
            P.dst[k] = (float4*)streams[k].dst;
            P.words[k] = streams[k].words;
        }
        P.index = index;
        P.count = count;
        P.tiles = compact_tiles(n);
        P.bits = (unsigned long long*)q.scratch.p;
        P.tile_count = (uint32_t*)(P.bits + (size_t)P.tiles * kCompactSegs);
        P.n_count = cnt.dev;
        P.n = n;
        P.mask = mask;
        P.streams = stream_count;
        launch_compact(P, std::min(path_resident_blocks(), P.tiles), stream);   // one block per tile at the most
        return RT_OK;
    });
}

rt_status connect_paths(rt_ctx* c, rt_path* paths, uint32_t n, const float* contrib, const uint32_t* index,
                        const uint32_t* occluded, Count cnt, QueryStream where) {
    const uint32_t m = cnt.n;
    if (!c) FAIL(c, RT_ERR_INVALID_ARG, "null ctx");
    if (m > 0 && n > 0) {
        if (!paths || !contrib || !occluded) FAIL(c, RT_ERR_INVALID_ARG, "null argument");
        if ((((uintptr_t)paths | (uintptr_t)contrib) & 15u) || (((uintptr_t)index | (uintptr_t)occluded) & 3u))
            FAIL(c, RT_ERR_INVALID_ARG, "paths and contrib must be 16-byte aligned, index and occluded 4-byte aligned");
    }
    if (m == 0 || n == 0) return RT_OK;
    return enqueue_query(c, where, false, [&](QuerySlot&, const Geo&, hipStream_t stream) -> rt_status {
        const ConnectParams P{(float4*)paths, (const float4*)contrib, index, occluded, cnt.dev, n, m};
        launch_connect(P, query_grid(path_resident_blocks(), m), stream);
        return RT_OK;
    });
}

rt_status retire_paths(rt_ctx* c, const rt_path* paths, Count cnt, float* samples, uint32_t tags, QueryStream where) {
    const uint32_t n = cnt.n;
    if (!c) FAIL(c, RT_ERR_INVALID_ARG, "null ctx");
    if (n > 0 && tags > 0) {
        if (!paths || !samples) FAIL(c, RT_ERR_INVALID_ARG, "null argument");
        if (((uintptr_t)paths | (uintptr_t)samples) & 15u) FAIL(c, RT_ERR_INVALID_ARG, "paths and samples must be 16-byte aligned");
    }
    if (n == 0 || tags == 0) return RT_OK;
    return enqueue_query(c, where, false, [&](QuerySlot&, const Geo&, hipStream_t stream) -> rt_status {
        const RetireParams P{(const float4*)paths, (float4*)samples, cnt.dev, n, tags};
        launch_retire(P, query_grid(path_resident_blocks(), n), stream);
        return RT_OK;
    });
}

rt_status average_samples(rt_ctx* c, const float* samples, uint32_t pixels, uint32_t spp, float* rgba, QueryStream where) {
    if (!c) FAIL(c, RT_ERR_INVALID_ARG, "null ctx");
    if (spp < 1 || spp > 64) FAIL(c, RT_ERR_INVALID_ARG, "spp outside 1 .. 64");
    if (pixels > 0) {
        if (!samples || !rgba) FAIL(c, RT_ERR_INVALID_ARG, "null argument");
        if (((uintptr_t)samples | (uintptr_t)rgba) & 15u) FAIL(c, RT_ERR_INVALID_ARG, "samples and rgba must be 16-byte aligned");
        if (samples == rgba) FAIL(c, RT_ERR_INVALID_ARG, "in place is not supported");
    }
    if (pixels == 0) return RT_OK;
    return enqueue_query(c, where, false, [&](QuerySlot&, const Geo&, hipStream_t stream) -> rt_status {
        const AverageParams P{(const float4*)samples, (float4*)rgba, pixels, spp};
        launch_average(P, query_grid(path_resident_blocks(), pixels), stream);
        return RT_OK;
    });
}
}  // namespace

rt_status drain_queries(rt_ctx* c) {
    for (int i = 0; i < kQuerySlots; ++i)   // qnext is the oldest slot
        if (rt_status st = harvest_query(c, (c->qnext + i) % kQuerySlots)) return st;
    return RT_OK;
}

extern "C" {

rt_status rt_trace_closest(rt_ctx* c, const rt_ray* rays, uint32_t n, rt_ray_hit* hits) {
    return trace(c, rays, n, hits, false, QueryStream::of_ctx());
}

rt_status rt_trace_any(rt_ctx* c, const rt_ray* rays, uint32_t n, uint32_t* occluded) {
    return trace(c, rays, n, occluded, true, QueryStream::of_ctx());
}

rt_status rt_trace_closest_on(rt_ctx* c, const rt_ray* rays, uint32_t n, rt_ray_hit* hits, void* stream) {
    return trace(c, rays, n, hits, false, QueryStream::on(stream));
}

rt_status rt_trace_any_on(rt_ctx* c, const rt_ray* rays, uint32_t n, uint32_t* occluded, void* stream) {
    return trace(c, rays, n, occluded, true, QueryStream::on(stream));
}

rt_status rt_resolve_hits(rt_ctx* c, const rt_ray* rays, const rt_ray_hit* hits, uint32_t n, rt_surface* surfaces,
                          rt_surface_material* materials) {
    return resolve(c, rays, hits, n, surfaces, materials, QueryStream::of_ctx());
}

rt_status rt_resolve_hits_on(rt_ctx* c, const rt_ray* rays, const rt_ray_hit* hits, uint32_t n, rt_surface* surfaces,
                             rt_surface_material* materials, void* stream) {
    return resolve(c, rays, hits, n, surfaces, materials, QueryStream::on(stream));
}

rt_status rt_shade_hits(rt_ctx* c, const rt_shade_opts* opts, const rt_ray* rays, const rt_surface* surfaces,
                        const rt_surface_material* materials, const float* randoms, uint32_t n, rt_path* paths,
                        rt_ray* next_rays, rt_ray* shadow_rays, float* contrib) {
    return shade(c, opts, rays, surfaces, materials, randoms, n, paths, next_rays, shadow_rays, contrib,
                 QueryStream::of_ctx());
}

rt_status rt_shade_hits_on(rt_ctx* c, const rt_shade_opts* opts, const rt_ray* rays, const rt_surface* surfaces,
                           const rt_surface_material* materials, const float* randoms, uint32_t n, rt_path* paths,
                           rt_ray* next_rays, rt_ray* shadow_rays, float* contrib, void* stream) {
    return shade(c, opts, rays, surfaces, materials, randoms, n, paths, next_rays, shadow_rays, contrib,
                 QueryStream::on(stream));
}

rt_status rt_camera_paths(rt_ctx* c, const Uniforms* u, const rt_camera_opts* opts, const uint32_t* random_offsets,
                          uint32_t n, rt_ray* rays, rt_path* paths) {
    return camera_paths(c, u, opts, random_offsets, n, rays, paths, QueryStream::of_ctx());
}

rt_status rt_camera_paths_on(rt_ctx* c, const Uniforms* u, const rt_camera_opts* opts, const uint32_t* random_offsets,
                             uint32_t n, rt_ray* rays, rt_path* paths, void* stream) {
    return camera_paths(c, u, opts, random_offsets, n, rays, paths, QueryStream::on(stream));
}

rt_status rt_compact_paths(rt_ctx* c, const rt_path* paths, uint32_t n, uint32_t mask, const rt_compact_stream* streams,
                           uint32_t stream_count, uint32_t* index, uint32_t* count) {
    return compact_paths(c, paths, n, mask, streams, stream_count, index, count, QueryStream::of_ctx());
}

rt_status rt_compact_paths_on(rt_ctx* c, const rt_path* paths, uint32_t n, uint32_t mask, const rt_compact_stream* streams,
                              uint32_t stream_count, uint32_t* index, uint32_t* count, void* stream) {
    return compact_paths(c, paths, n, mask, streams, stream_count, index, count, QueryStream::on(stream));
}

rt_status rt_connect_paths(rt_ctx* c, rt_path* paths, uint32_t n, const float* contrib, const uint32_t* index,
                           const uint32_t* occluded, uint32_t m) {
    return connect_paths(c, paths, n, contrib, index, occluded, m, QueryStream::of_ctx());
}

rt_status rt_connect_paths_on(rt_ctx* c, rt_path* paths, uint32_t n, const float* contrib, const uint32_t* index,
                              const uint32_t* occluded, uint32_t m, void* stream) {
    return connect_paths(c, paths, n, contrib, index, occluded, m, QueryStream::on(stream));
}

rt_status rt_retire_paths(rt_ctx* c, const rt_path* paths, uint32_t n, float* samples, uint32_t tags) {
    return retire_paths(c, paths, n, samples, tags, QueryStream::of_ctx());
}

rt_status rt_retire_paths_on(rt_ctx* c, const rt_path* paths, uint32_t n, float* samples, uint32_t tags, void* stream) {
    return retire_paths(c, paths, n, samples, tags, QueryStream::on(stream));
}

rt_status rt_average_samples(rt_ctx* c, const float* samples, uint32_t pixels, uint32_t spp, float* rgba) {
    return average_samples(c, samples, pixels, spp, rgba, QueryStream::of_ctx());
}

rt_status rt_average_samples_on(rt_ctx* c, const float* samples, uint32_t pixels, uint32_t spp, float* rgba, void* stream) {
    return average_samples(c, samples, pixels, spp, rgba, QueryStream::on(stream));
}

// The _indirect forms: the direct form's function with the device count checked and handed on.
rt_status rt_trace_closest_indirect(rt_ctx* c, const rt_ray* rays, const rt_device_count* cnt, rt_ray_hit* hits) {
    return with_device_count(c, cnt, [&](Count n) { return trace(c, rays, n, hits, false, QueryStream::of_ctx()); });
}

rt_status rt_trace_closest_on_indirect(rt_ctx* c, const rt_ray* rays, const rt_device_count* cnt, rt_ray_hit* hits,
                                       void* stream) {
    return with_device_count(c, cnt, [&](Count n) { return trace(c, rays, n, hits, false, QueryStream::on(stream)); });
}

rt_status rt_trace_any_indirect(rt_ctx* c, const rt_ray* rays, const rt_device_count* cnt, uint32_t* occluded) {
    return with_device_count(c, cnt, [&](Count n) { return trace(c, rays, n, occluded, true, QueryStream::of_ctx()); });
}

rt_status rt_trace_any_on_indirect(rt_ctx* c, const rt_ray* rays, const rt_device_count* cnt, uint32_t* occluded,
                                   void* stream) {
    return with_device_count(c, cnt, [&](Count n) { return trace(c, rays, n, occluded, true, QueryStream::on(stream)); });
}

rt_status rt_resolve_hits_indirect(rt_ctx* c, const rt_ray* rays, const rt_ray_hit* hits, const rt_device_count* cnt,
                                   rt_surface* surfaces, rt_surface_material* materials) {
    return with_device_count(
        c, cnt, [&](Count n) { return resolve(c, rays, hits, n, surfaces, materials, QueryStream::of_ctx()); });
}

rt_status rt_resolve_hits_on_indirect(rt_ctx* c, const rt_ray* rays, const rt_ray_hit* hits, const rt_device_count* cnt,
                                      rt_surface* surfaces, rt_surface_material* materials, void* stream) {
    return with_device_count(
        c, cnt, [&](Count n) { return resolve(c, rays, hits, n, surfaces, materials, QueryStream::on(stream)); });
}

rt_status rt_shade_hits_indirect(rt_ctx* c, const rt_shade_opts* opts, const rt_ray* rays, const rt_surface* surfaces,
                                 const rt_surface_material* materials, const float* randoms, const rt_device_count* cnt,
                                 rt_path* paths, rt_ray* next_rays, rt_ray* shadow_rays, float* contrib) {
    return with_device_count(c, cnt, [&](Count n) {
        return shade(c, opts, rays, surfaces, materials, randoms, n, paths, next_rays, shadow_rays, contrib,
                     QueryStream::of_ctx());
    });
}

rt_status rt_shade_hits_on_indirect(rt_ctx* c, const rt_shade_opts* opts, const rt_ray* rays, const rt_surface* surfaces,
                                    const rt_surface_material* materials, const float* randoms, const rt_device_count* cnt,
                                    rt_path* paths, rt_ray* next_rays, rt_ray* shadow_rays, float* contrib, void* stream) {
    return with_device_count(c, cnt, [&](Count n) {
        return shade(c, opts, rays, surfaces, materials, randoms, n, paths, next_rays, shadow_rays, contrib,
                     QueryStream::on(stream));
    });
}

rt_status rt_compact_paths_indirect(rt_ctx* c, const rt_path* paths, const rt_device_count* cnt, uint32_t mask,
                                    const rt_compact_stream* streams, uint32_t stream_count, uint32_t* index,
                                    uint32_t* count) {
    return with_device_count(c, cnt, [&](Count n) {
        return compact_paths(c, paths, n, mask, streams, stream_count, index, count, QueryStream::of_ctx());
    });
}

rt_status rt_compact_paths_on_indirect(rt_ctx* c, const rt_path* paths, const rt_device_count* cnt, uint32_t mask,
                                       const rt_compact_stream* streams, uint32_t stream_count, uint32_t* index,
                                       uint32_t* count, void* stream) {
    return with_device_count(c, cnt, [&](Count n) {
        return compact_paths(c, paths, n, mask, streams, stream_count, index, count, QueryStream::on(stream));
    });
}

rt_status rt_connect_paths_indirect(rt_ctx* c, rt_path* paths, uint32_t n, const float* contrib, const uint32_t* index,
                                    const uint32_t* occluded, const rt_device_count* cnt) {
    return with_device_count(
        c, cnt, [&](Count m) { return connect_paths(c, paths, n, contrib, index, occluded, m, QueryStream::of_ctx()); });
}

rt_status rt_connect_paths_on_indirect(rt_ctx* c, rt_path* paths, uint32_t n, const float* contrib, const uint32_t* index,
                                       const uint32_t* occluded, const rt_device_count* cnt, void* stream) {
    return with_device_count(
        c, cnt, [&](Count m) { return connect_paths(c, paths, n, contrib, index, occluded, m, QueryStream::on(stream)); });
}

rt_status rt_retire_paths_indirect(rt_ctx* c, const rt_path* paths, const rt_device_count* cnt, float* samples,
                                   uint32_t tags) {
    return with_device_count(c, cnt, [&](Count n) { return retire_paths(c, paths, n, samples, tags, QueryStream::of_ctx()); });
}

rt_status rt_retire_paths_on_indirect(rt_ctx* c, const rt_path* paths, const rt_device_count* cnt, float* samples,
                                      uint32_t tags, void* stream) {
    return with_device_count(c, cnt, [&](Count n) { return retire_paths(c, paths, n, samples, tags, QueryStream::on(stream)); });
}

rt_status rt_get_query_stats(rt_ctx* c, rt_query_stats* out) {
    if (!c || !out) FAIL(c, RT_ERR_INVALID_ARG, "null argument");
    HIPC(c, hipSetDevice(c->device));
    if (rt_status st = drain_queries(c)) return st;
    *out = c->qstats;
    if (c->q_overflow) {
        c->q_overflow = false;
        FAIL(c, RT_ERR_STATE, "traversal stack overflow in a ray query");
    }
    return RT_OK;
}

}  // extern "C"
