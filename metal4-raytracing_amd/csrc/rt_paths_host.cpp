// rt_paths_host.cpp — the host hooks of the path queries: rt_debug_camera_paths_host runs
// camera_record (rt_paths.h), the code rq_camera runs, compiled for the host, with the Halton
// table rt_create uploads; rt_debug_compact_paths_host is rt_compact_paths as a sequential loop.
// Both make the device calls' own checks (rt_scene_host.h).  No device call is made: the file
// also links into stand-alone host programs, as rt_scatter_host.cpp does.
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
