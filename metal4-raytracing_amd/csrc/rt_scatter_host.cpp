// rt_scatter_host.cpp — rt_debug_shade_host: the shading query (rt_shade_hits) over host arrays.
// It makes the Halton table rt_create uploads and runs scatter_eval (rt_scatter.h), compiled for
// the host, over the records with the caller's lights.  No device call is made: the file also
// links into stand-alone host programs, as rt_surface_host.cpp does.
#include <exception>

#include "rt_scatter.h"
#include "rt_scene_host.h"

using namespace rt;

extern "C" rt_status rt_debug_shade_host(const Light* lights, uint32_t light_count, const rt_shade_opts* opts,
                                         const rt_ray* rays, const rt_surface* surfaces,
                                         const rt_surface_material* materials, const float* randoms, uint32_t n,
                                         rt_path* paths, rt_ray* next_rays, rt_ray* shadow_rays, float* contrib) {
    rt_ctx* const none = nullptr;
    if (rt_status st = validate_shade(none, opts, rays, surfaces, materials, randoms, n, paths, next_rays, shadow_rays, contrib))
        return st;
    if (!lights && light_count) FAIL(none, RT_ERR_INVALID_ARG, "null lights");
    ScatterOpts U{opts->shading_mode, opts->max_bounces, 0};
    if (rt_status st = shade_light_count(none, opts, light_count, U.lightCount)) return st;
    try {
        std::vector<HaltonDim> tab(RT_HALTON_DIMS);
        halton_table_fill(tab.data(), RT_HALTON_DIMS);
        for (uint32_t i = 0; i < n; ++i) {
            float4 d4, s[4], m[3], r[2] = {make_float4(0.0f, 0.0f, 0.0f, 0.0f), make_float4(0.0f, 0.0f, 0.0f, 0.0f)};
            std::memcpy(&d4, &rays[i].direction, 16);
            std::memcpy(s, &surfaces[i], 64);
            std::memcpy(m, &materials[i], 48);
            if (randoms) std::memcpy(r, randoms + 8 * (size_t)i, 32);
            PathWords w;
            std::memcpy(&w, &paths[i], 48);
            ScatterOut o;
            const uint4 s3 = __builtin_bit_cast(uint4, s[3]);
            if (randoms) scatter_eval<true>(tab.data(), lights, U, d4, s[0], s[1], s[2], s3, m[0], m[1], m[2], r[0], r[1], w, o);
            else scatter_eval<false>(tab.data(), lights, U, d4, s[0], s[1], s[2], s3, m[0], m[1], m[2], r[0], r[1], w, o);
            std::memcpy(&paths[i], &w, 48);
            std::memcpy(&next_rays[i], &o.n0, 32);
            std::memcpy(&shadow_rays[i], &o.h0, 32);
            std::memcpy(contrib + 4 * (size_t)i, &o.c, 16);
        }
    } catch (const std::exception&) {   // nothing is thrown across the C-ABI
        FAIL(none, RT_ERR_OUT_OF_MEMORY, "rt_debug_shade_host: allocation failed");
    }
    return RT_OK;
}
