// surface_host_check.cpp — rt_debug_resolve_host (csrc/rt_surface_host.cpp, csrc/rt_surface.h) as a
// stand-alone host program, for a build under AddressSanitizer + UBSan (tools/surface_host_check.sh):
// hit records whose triangle id is in range resolve to that triangle, and records whose id is the
// triangle count, 0xfffffffe or RT_MISS resolve to the miss record without indexing anything.  The
// scene is made here: a textured quad (base-colour and normal map, with UVs) and one plain triangle.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../include/rt_api.h"

thread_local std::string rt_g_err;   // the library's rt_last_error(NULL) text (rt_api.cpp there)

static int fail(const char* what, unsigned k) {
    std::printf("surface_host_check: FAILED: %s (record %u): %s\n", what, k, rt_g_err.c_str());
    return 1;
}

int main() {
    // mesh 0: a unit quad in the plane y = 0, two triangles, UVs, maps bound; mesh 1: one triangle at y = 1
    const rt_float3 qpos[4] = {{0, 0, 0, 0}, {1, 0, 0, 0}, {1, 0, 1, 0}, {0, 0, 1, 0}};
    const rt_float3 qnrm[4] = {{0, 1, 0, 0}, {0, 1, 0, 0}, {0, 1, 0, 0}, {0, 1, 0, 0}};
    const rt_float2 quv[4] = {{0, 0}, {1, 0}, {1, 1}, {0, 1}};
    const uint32_t qidx[6] = {0, 1, 2, 0, 2, 3};
    const rt_float3 tpos[3] = {{0, 1, 0, 0}, {1, 1, 0, 0}, {0, 1, 1, 0}};
    const rt_float3 tnrm[3] = {{0, 1, 0, 0}, {0, 1, 0, 0}, {0, 0, 0, 0}};
    const uint32_t tidx[3] = {0, 1, 2};
    std::vector<uint8_t> texels(4 * 4 * 4);
    for (size_t i = 0; i < texels.size(); ++i) texels[i] = (uint8_t)(37 * i + 11);
    const rt_texture_desc tex[1] = {{texels.data(), 4, 4}};
    rt_submesh_desc qsub, tsub;
    std::memset(&qsub, 0, sizeof qsub);
    std::memset(&tsub, 0, sizeof tsub);
    qsub.indices = qidx;
    qsub.index_count = 6;
    qsub.material.baseColor = {1, 1, 1, 0};
    qsub.material.opacity = 1.0f;
    qsub.material.refractionIndex = 1.0f;
    qsub.material.textureFlags = MATERIAL_TEXTURE_BASECOLOR | MATERIAL_TEXTURE_NORMAL | MATERIAL_TEXTURE_OPACITY;
    for (int k = 0; k < 8; ++k) qsub.textures[k] = 0;
    tsub.indices = tidx;
    tsub.index_count = 3;
    tsub.material.baseColor = {0.5f, 0.25f, 0.125f, 0};
    tsub.material.opacity = 0.5f;
    tsub.material.refractionIndex = 1.5f;
    for (int k = 0; k < 8; ++k) tsub.textures[k] = -1;
    rt_mesh_desc meshes[2];
    std::memset(meshes, 0, sizeof meshes);
    const rt_packed_float4x3 ident = {{{1, 0, 0}, {0, 1, 0}, {0, 0, 1}, {0, 0, 0}}};
    meshes[0].positions = qpos;
    meshes[0].normals = qnrm;
    meshes[0].uvs = quv;
    meshes[0].vertex_count = 4;
    meshes[0].submesh_count = 1;
    meshes[0].submeshes = &qsub;
    meshes[0].transform = ident;
    meshes[1].positions = tpos;
    meshes[1].normals = tnrm;
    meshes[1].vertex_count = 3;
    meshes[1].submesh_count = 1;
    meshes[1].submeshes = &tsub;
    meshes[1].transform = ident;
    Light light;
    std::memset(&light, 0, sizeof light);
    light.type = LightTypePointlight;
    rt_scene_desc sd;
    std::memset(&sd, 0, sizeof sd);
    sd.mesh_count = 2;
    sd.light_count = 1;
    sd.meshes = meshes;
    sd.lights = &light;
    sd.texture_count = 1;
    sd.textures = tex;

    const uint32_t ntris = 3;
    const uint32_t ids[] = {0, 1, 2, ntris, ntris + 1, 0xfffffffeu, RT_MISS, 0x80000000u, 2, 0};
    const uint32_t n = sizeof ids / sizeof ids[0];
    // exactly n records each, on the heap: a read or a write past either end is a report
    std::vector<rt_ray> rays(n);
    std::vector<rt_ray_hit> hits(n);
    std::vector<rt_surface> surf(n);
    std::vector<rt_surface_material> mat(n);
    for (uint32_t k = 0; k < n; ++k) {
        rays[k] = rt_ray{{0.25f, 2.0f, 0.25f}, 0.0f, {0.0f, -1.0f, 0.0f}, INFINITY};
        hits[k] = rt_ray_hit{1.0f + (float)k, 0.25f, 0.5f, ids[k], 7u, 9u, 11u, 0u};   // mesh / submesh: copied, never indexed with
    }
    for (int with_mat = 1; with_mat >= 0; --with_mat) {
        std::memset(surf.data(), 0xab, n * sizeof(rt_surface));
        std::memset(mat.data(), 0xab, n * sizeof(rt_surface_material));
        if (rt_debug_resolve_host(&sd, rays.data(), hits.data(), n, surf.data(), with_mat ? mat.data() : nullptr) != RT_OK)
            return fail("rt_debug_resolve_host", 0);
        for (uint32_t k = 0; k < n; ++k) {
            const rt_surface& s = surf[k];
            uint32_t mw[12];
            std::memcpy(mw, &mat[k], 48);
            if (ids[k] < ntris) {
                if (s.triangle != ids[k] || s.mesh != 7u || s.submesh != 9u || s.t != 1.0f + (float)k) return fail("hit ids", k);
                if (s.position[1] != 2.0f - s.t) return fail("hit position", k);
                const bool quad = ids[k] < 2;
                if (((s.flags & RT_SURFACE_HAS_UV) != 0) != quad) return fail("uv flag", k);
                if (!quad && !(s.flags & RT_SURFACE_TRANSMISSIVE)) return fail("transmissive flag", k);
                if (with_mat && mat[k].slot != (quad ? 0u : 1u)) return fail("material slot", k);
            } else {
                if (s.triangle != RT_MISS || s.mesh != RT_MISS || s.submesh != RT_MISS || s.flags != 0 || !std::isinf(s.t))
                    return fail("miss record", k);
                for (int j = 0; j < 3; ++j)
                    if (s.position[j] != 0.0f || s.normal[j] != 0.0f || s.shading_normal[j] != 0.0f) return fail("miss zeros", k);
                if (s.u != 0.0f || s.v != 0.0f) return fail("miss uv", k);
                for (int j = 0; j < 12; ++j)
                    if (with_mat && mw[j] != 0u) return fail("miss material", k);
            }
            for (int j = 0; j < 12; ++j)
                if (!with_mat && mw[j] != 0xababababu) return fail("material written without being asked for", k);
        }
    }
    // the checks of the entry point itself
    if (rt_debug_resolve_host(nullptr, rays.data(), hits.data(), n, surf.data(), nullptr) != RT_ERR_INVALID_ARG) return fail("null scene", 0);
    if (rt_debug_resolve_host(&sd, rays.data(), nullptr, n, surf.data(), nullptr) != RT_ERR_INVALID_ARG) return fail("null hits", 0);
    if (rt_debug_resolve_host(&sd, nullptr, nullptr, 0, nullptr, nullptr) != RT_OK) return fail("n = 0", 0);
    qsub.textures[1] = 5;   // a flagged slot without a texture: refused as rt_scene_upload refuses it
    if (rt_debug_resolve_host(&sd, rays.data(), hits.data(), n, surf.data(), nullptr) != RT_ERR_INVALID_ARG) return fail("bad texture id", 0);
    std::printf("surface_host_check: ok (%u records, %u of them out of range)\n", n, 5u);
    return 0;
}
