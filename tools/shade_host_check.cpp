// shade_host_check.cpp — rt_debug_shade_host (csrc/rt_scatter_host.cpp, csrc/rt_scatter.h) as a
// stand-alone host program, for a build under AddressSanitizer + UBSan (tools/shade_host_check.sh):
// a caller's light numbers outside [0, 1) (negative, 1, 2, huge, infinite, NaN) pick a light inside
// the array, a caller's step far past the renderer's (and a negative one) reads a Halton dimension
// inside the table, and dead, missed and spent records touch nothing.  Every array holds exactly n
// records on the heap, the lights exactly `count`: a read or a write past an end is a report.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../include/rt_api.h"

thread_local std::string rt_g_err;   // the library's rt_last_error(NULL) text (rt_api.cpp there)

static int fail(const char* what, unsigned k) {
    std::printf("shade_host_check: FAILED: %s (record %u): %s\n", what, k, rt_g_err.c_str());
    return 1;
}

int main() {
    const uint32_t count = 3;
    std::vector<Light> lights(count);
    std::memset(lights.data(), 0, count * sizeof(Light));
    lights[0].type = LightTypeAreaLight;
    lights[0].position = {0, 2, 0, 0};
    lights[0].color = {4, 4, 4, 0};
    lights[0].forward = {0, -1, 0, 0};
    lights[0].right = {0.25f, 0, 0, 0};
    lights[0].up = {0, 0, 0.25f, 0};
    lights[1].type = LightTypeSpotlight;
    lights[1].position = {2, 1, 4, 0};
    lights[1].color = {4, 4, 4, 0};
    lights[1].direction = {-1.5f, -0.5f, -1.5f, 0};
    lights[1].coneAngle = 0.436f;
    lights[2].type = LightTypeSunlight;
    lights[2].color = {1, 1, 1, 0};
    lights[2].direction = {-1, -2, 0, 0};

    const float light_x[] = {0.1f, 0.5f, 0.9f, -1.0f, 1.0f, 2.0f, 3.0e9f, -3.0e9f, INFINITY, -INFINITY, NAN, 0.999999f};
    const int steps[] = {0, 1, 11, 156, 170, 171, 1 << 20, 0x7ffffff0, -1, -5, -0x7ffffff0, 3};
    const uint32_t n = sizeof light_x / sizeof light_x[0];
    std::vector<rt_ray> rays(n), next(n), shadow(n);
    std::vector<rt_surface> surf(n);
    std::vector<rt_surface_material> mat(n);
    std::vector<rt_path> paths(n);
    std::vector<float> rnd(8 * (size_t)n), contrib(4 * (size_t)n);
    rt_shade_opts opts;
    std::memset(&opts, 0, sizeof opts);
    opts.max_bounces = 12;
    for (int with_rnd = 0; with_rnd < 2; ++with_rnd)
        for (int mode = 0; mode < 2; ++mode)
            for (int glass = 0; glass < 2; ++glass) {
                opts.shading_mode = mode;
                for (uint32_t k = 0; k < n; ++k) {
                    rays[k] = rt_ray{{0.25f, 2.0f, 0.25f}, 0.0f, {0.0f, -1.0f, 0.0f}, INFINITY};
                    surf[k] = rt_surface{{0.25f, 0.0f, 0.25f}, 2.0f, {0, 1, 0}, 0.0f, {0, 1, 0}, 0.0f, 0u, 0u, 0u, 0u};
                    mat[k] = rt_surface_material{{0.8f, 0.7f, 0.6f}, glass ? 0.08f : 1.0f, {0, 0, 0}, glass ? 1.52f : 1.0f,
                                                 1.0f, 0.0f, 0u, 0u};
                    paths[k] = rt_path{{1, 1, 1}, 12345u + k, {0, 0, 0}, RT_PATH_ALIVE, 0, steps[k], 0, 0u};
                    const float r[8] = {light_x[k], 0.3f, 0.7f, 0.5f, 0.25f, 0.75f, 0.0f, 0.0f};
                    std::memcpy(&rnd[8 * (size_t)k], r, sizeof r);
                }
                if (rt_debug_shade_host(lights.data(), count, &opts, rays.data(), surf.data(), mat.data(),
                                        with_rnd ? rnd.data() : nullptr, n, paths.data(), next.data(), shadow.data(),
                                        contrib.data()) != RT_OK)
                    return fail("rt_debug_shade_host", 0);
                for (uint32_t k = 0; k < n; ++k) {
                    if (paths[k].step != steps[k] + 1) return fail("step", k);
                    if (!(paths[k].flags & RT_PATH_ALIVE) || !std::isinf(next[k].tmax)) return fail("next ray", k);
                    if (glass && (paths[k].flags & RT_PATH_SHADOW)) return fail("glass shadow", k);
                    if (!(paths[k].flags & RT_PATH_SHADOW) && shadow[k].tmax != -1.0f) return fail("no-shadow fill", k);
                }
            }
    // dead, missed and spent records: only the flag bits change, the outputs are the zero fill
    for (uint32_t k = 0; k < n; ++k) {
        paths[k] = rt_path{{1, 1, 1}, 7u, {0.5f, 0.5f, 0.5f}, (k % 3 == 0 ? 0u : RT_PATH_ALIVE) | RT_PATH_SHADOW,
                           k % 3 == 1 ? 12 : 0, 2, 1, 0u};
        if (k % 3 == 2) surf[k].triangle = RT_MISS;
    }
    if (rt_debug_shade_host(lights.data(), count, &opts, rays.data(), surf.data(), mat.data(), nullptr, n, paths.data(),
                            next.data(), shadow.data(), contrib.data()) != RT_OK)
        return fail("rt_debug_shade_host (unshaded records)", 0);
    for (uint32_t k = 0; k < n; ++k) {
        if (paths[k].flags != 0u || paths[k].step != 2 || paths[k].radiance[0] != 0.5f) return fail("unshaded path", k);
        if (next[k].tmax != -1.0f || shadow[k].tmax != -1.0f || contrib[4 * k] != 0.0f) return fail("unshaded outputs", k);
    }
    // the checks of the entry point itself
    if (rt_debug_shade_host(lights.data(), count, nullptr, rays.data(), surf.data(), mat.data(), nullptr, n, paths.data(),
                            next.data(), shadow.data(), contrib.data()) != RT_ERR_INVALID_ARG) return fail("null opts", 0);
    opts.light_count = (int32_t)count + 1;
    if (rt_debug_shade_host(lights.data(), count, &opts, rays.data(), surf.data(), mat.data(), nullptr, n, paths.data(),
                            next.data(), shadow.data(), contrib.data()) != RT_ERR_INVALID_ARG) return fail("light count", 0);
    opts.light_count = 0;
    if (rt_debug_shade_host(lights.data(), count, &opts, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr,
                            nullptr) != RT_OK) return fail("n = 0", 0);
    std::printf("shade_host_check: ok (%u records x 8 variants)\n", n);
    return 0;
}
