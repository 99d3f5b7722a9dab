// rt_paths_host.cpp — the host hooks of the path queries: rt_debug_camera_paths_host runs
// camera_record (rt_paths.h), the code rq_camera runs, compiled for the host, with the Halton
// table rt_create uploads; rt_debug_compact_paths_host is rt_compact_paths as a sequential loop.
// rt_debug_primary_outputs_host, rt_debug_extra_paths_host and rt_debug_resolve_samples_host run the
// temporal per-record code (rt_paths.h, around rt_shade.h's primary_outputs, extra_samples and
// resolve_pixel) the same way; they have no device call yet.
// All make their checks through rt_scene_host.h (the path hooks: the device calls' own).  No device
// call is made: the file also links into stand-alone host programs, as rt_scatter_host.cpp does.
#include <exception>

#include "rt_paths.h"
#include "rt_scene_host.h"

using namespace rt;

extern "C" rt_status rt_debug_camera_paths_host(const Uniforms* u, const rt_camera_opts* opts,
                                                const uint32_t* random_offsets, uint32_t n, rt_ray* rays,
                                                rt_path* paths) {
    rt_ctx* const none = nullptr;
    if (rt_status st = validate_camera(none, u, opts, random_offsets, n, rays, paths)) return st;
    if (!random_offsets) FAIL(none, RT_ERR_INVALID_ARG, "null random_offsets");
    HaltonDim tab[2];
    halton_table_fill(tab, 2);
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t pix = opts->first_pixel + i;
        CameraWords w;
        camera_record(*u, tab[1], random_offsets[pix], pix, opts->sample, pix * opts->tag_stride + opts->tag_offset, w);
        std::memcpy(&rays[i], &w.r0, 32);
        std::memcpy(&paths[i], &w.p0, 48);
    }
    return RT_OK;
}

// The temporal hooks: loops over host arrays around the per-record functions of rt_paths.h.
extern "C" rt_status rt_debug_primary_outputs_host(const rt_scene_desc* sd, const rt_packed_float4x3* prev_transforms,
                                                   const Uniforms* u, const rt_target_opts* opts, const rt_ray_hit* hits,
                                                   const rt_path* paths, uint32_t n, float* depth, float* motion) {
    rt_ctx* const none = nullptr;
    if (!sd) FAIL(none, RT_ERR_INVALID_ARG, "null scene");
    if (rt_status st = validate_primary(none, u, opts, hits, paths, n, depth, motion)) return st;
    int max_sub = 1;
    uint64_t nv = 0, nt = 0;
    if (rt_status st = validate_scene(none, sd, max_sub, nv, nt)) return st;
    if (n == 0) return RT_OK;
    try {
        std::vector<float4> pos;
        std::vector<uint4> tri_info;
        std::vector<float> inst;
        flatten_scene(sd, pos, nullptr, tri_info, inst);
        std::vector<float> prev_inst = inst;
        if (prev_transforms) std::memcpy(prev_inst.data(), prev_transforms, 48 * (size_t)sd->mesh_count);
        DevScene S;
        std::memset(&S, 0, sizeof S);
        S.tri_info = tri_info.data();
        S.pos = pos.data();
        S.prev_pos = pos.data();   // previousPositions = positions, as after rt_scene_upload
        S.inst = inst.data();
        S.prev_inst = prev_inst.data();
        S.max_submeshes = max_sub;
        S.num_tris = (int)nt;
        for (uint32_t i = 0; i < n; ++i) {
            uint32_t pix = 0;
            if (!primary_selected(paths[i].flags, paths[i].bounce, paths[i].reserved, opts->tag_stride, opts->tag_offset,
                                  opts->pixels, pix))
                continue;
            float4 h0;
            std::memcpy(&h0, &hits[i], 16);
            float d;
            f2 mv;
            if (!primary_record(S, *u, h0, d, mv)) continue;
            depth[pix] = d;
            motion[2 * (size_t)pix] = mv.x;
            motion[2 * (size_t)pix + 1] = mv.y;
        }
    } catch (const std::exception&) {   // nothing is thrown across the C-ABI
        FAIL(none, RT_ERR_OUT_OF_MEMORY, "rt_debug_primary_outputs_host: allocation failed");
    }
    return RT_OK;
}

extern "C" rt_status rt_debug_extra_paths_host(const Uniforms* u, const rt_camera_opts* opts, const uint32_t* random_offsets,
                                               const float* motion, const float* motion_prev, uint32_t n, rt_ray* rays,
                                               rt_path* paths, uint32_t* extra) {
    rt_ctx* const none = nullptr;
    const int max_extra = u ? max_extra_samples(*u) : 0;
    if (rt_status st = validate_extra(none, u, opts, random_offsets, motion, motion_prev, n, rays, paths, extra, max_extra))
        return st;
    if (!random_offsets) FAIL(none, RT_ERR_INVALID_ARG, "null random_offsets");
    HaltonDim tab[2];
    halton_table_fill(tab, 2);
    const float2* const mv = reinterpret_cast<const float2*>(motion);
    const float2* const pm = reinterpret_cast<const float2*>(motion_prev);
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t pix = opts->first_pixel + i;
        const int e = extra_count(*u, ld2(mv, pix), ld2(pm, pix));
        extra[i] = (uint32_t)e;
        for (int j = 0; j < max_extra; ++j) {
            CameraWords w;
            if (j < e)
                camera_record(*u, tab[1], random_offsets[pix], pix, opts->sample + j,
                              pix * opts->tag_stride + opts->tag_offset + (uint32_t)j, w);
            else
                camera_record_none(w);
            const size_t r = (size_t)i * (size_t)max_extra + (size_t)j;
            std::memcpy(&rays[r], &w.r0, 32);
            std::memcpy(&paths[r], &w.p0, 48);
        }
    }
    return RT_OK;
}

extern "C" rt_status rt_debug_resolve_samples_host(const Uniforms* u, const float* samples, uint32_t sample_stride,
                                                   const uint32_t* extra, const float* motion, const float* motion_prev,
                                                   const float* history, uint32_t pixels, float* rgba) {
    rt_ctx* const none = nullptr;
    if (rt_status st = validate_resolve_samples(none, u, samples, sample_stride, extra, motion, motion_prev, history, pixels,
                                                rgba, u ? max_extra_samples(*u) : 0))
        return st;
    const float4* const s = reinterpret_cast<const float4*>(samples);
    const float2* const mv = reinterpret_cast<const float2*>(motion);
    const float2* const pm = reinterpret_cast<const float2*>(motion_prev);
    float4* const out = reinterpret_cast<float4*>(rgba);
    for (size_t p = 0; p < (size_t)pixels; ++p)
        out[p] = resolve_samples_pixel(*u, s + p * sample_stride,
                                       pixel_samples(extra, p, (uint32_t)u->samplesPerPixel, sample_stride), ld2(mv, p),
                                       ld2(pm, p), reinterpret_cast<const float4*>(history), p);
    return RT_OK;
}

extern "C" rt_status rt_debug_compact_paths_host(const rt_path* paths, uint32_t n, uint32_t mask,
                                                 const rt_compact_stream* streams, uint32_t stream_count,
                                                 uint32_t* index, uint32_t* count) {
    rt_ctx* const none = nullptr;
    if (rt_status st = validate_compact(none, paths, n, mask, streams, stream_count, index, count)) return st;
    if (n == 0) return RT_OK;
    uint32_t m = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if ((paths[i].flags & mask) == 0u) continue;
        for (uint32_t k = 0; k < stream_count; ++k) {
            const size_t bytes = 16 * (size_t)streams[k].words;
            std::memcpy((char*)streams[k].dst + bytes * m, (const char*)streams[k].src + bytes * i, bytes);
        }
        if (index) index[m] = i;
        ++m;
    }
    *count = m;
    return RT_OK;
}
