// Prints one 64-bit FNV-1a digest per buffer of the scenes the host ingest builds, so that two builds
// of the ingest can be compared line for line (profiles/r10_scene_split.txt):
//   scene_digest <asset dir> <inputs dir>
// <asset dir> holds the unpacked preset assets (assets/), <inputs dir> what
// tools/scene_digest_inputs.py wrote.  Host code only; build it as tools/fuzz_host.sh builds its
// program, from tools/scene_digest.cpp and the host sources of the library.
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../include/rt_scene.h"

static uint64_t fnv(const void* p, size_t n, uint64_t h = 0xcbf29ce484222325ull) {
    const uint8_t* b = (const uint8_t*)p;
    for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 0x100000001b3ull;
    return h;
}
// one "name=digest/bytes" token per buffer; a null buffer digests as 0
static void tok(const std::string& name, const void* p, size_t n) {
    std::printf(" %s=%016llx/%zu", name.c_str(), (unsigned long long)(p ? fnv(p, n) : 0), n);
}
static void line(const std::string& what, const void* p, size_t n) {
    std::printf("  %s", what.c_str());
    tok("", p, n);
    std::printf("\n");
}

static void digest(const char* label, rt_status st, rt_scene* s) {
    std::printf("%s: status %d, error \"%s\"\n", label, (int)st, s ? rt_scene_last_error(s) : "");
    rt_scene_desc d;
    if (st != RT_OK || rt_scene_get_desc(s, &d) != RT_OK) return;
    std::printf("  meshes %u, lights %u, textures %u, triangles %llu\n", d.mesh_count, d.light_count, d.texture_count,
                (unsigned long long)rt_scene_triangle_count(s));
    for (uint32_t m = 0; m < d.mesh_count; ++m) {
        const rt_mesh_desc& M = d.meshes[m];
        std::printf("  mesh%u:", m);
        tok("pos", M.positions, sizeof(rt_float3) * M.vertex_count);
        tok("nrm", M.normals, sizeof(rt_float3) * M.vertex_count);
        tok("uv", M.uvs, M.uvs ? sizeof(rt_float2) * M.vertex_count : 0);
        tok("ji", M.joint_indices, M.joint_indices ? 8 * (size_t)M.vertex_count : 0);
        tok("jw", M.joint_weights, M.joint_weights ? 16 * (size_t)M.vertex_count : 0);
        tok("xf", &M.transform, sizeof M.transform);
        tok("jc", &M.joint_count, sizeof M.joint_count);
        std::printf("\n");
        for (uint32_t k = 0; k < M.submesh_count; ++k) {
            const rt_submesh_desc& S = M.submeshes[k];
            std::printf("  mesh%u.sub%u:", m, k);
            tok("idx", S.indices, 4 * (size_t)S.index_count);
            tok("mat", &S.material, sizeof S.material);
            tok("tex", S.textures, sizeof S.textures);
            std::printf("\n");
        }
        if (M.joint_count == 0) continue;
        std::printf("  mesh%u.joints:", m);
        for (double t : {0.0, 0.37, 1.9}) {
            std::vector<float> J((size_t)M.joint_count * 16);
            uint32_t jc = 0;
            const rt_status js = rt_scene_joint_matrices(s, m, t, J.data(), M.joint_count, &jc);
            tok((js == RT_OK ? "t" : "FAILED_t") + std::to_string(t), J.data(), 64 * (size_t)jc);
        }
        std::printf("\n");
    }
    line("lights", d.lights, sizeof(Light) * d.light_count);
    for (uint32_t t = 0; t < d.texture_count; ++t) {
        const uint32_t wh[2] = {d.textures[t].width, d.textures[t].height};
        std::printf("  tex%u:", t);
        tok("size", wh, sizeof wh);
        tok("texels", d.textures[t].rgba8, 4 * (size_t)wh[0] * wh[1]);
        std::printf("\n");
    }
}

int main(int argc, char** argv) {
    if (argc < 3) {
        std::fprintf(stderr, "usage: %s <asset dir> <inputs dir>\n", argv[0]);
        return 2;
    }
    const std::string assets = argv[1], in = argv[2];
    const float zero[3] = {0, 0, 0}, pos[3] = {0.25f, -1.0f, 2.0f}, rot[3] = {0.1f, 0.7f, -0.3f};
    for (const char* name : {"c1", "c2", "c3g", "c3d", "c3k", "c3r", "c5", "app", "c2_synthetic", "c5_synthetic",
                             "app_synthetic", "nonesuch"}) {
        rt_scene* s = nullptr;
        int32_t synth = -1;
        const rt_status st = rt_scene_preset(name, assets.c_str(), &s, &synth);
        std::printf("preset %s (synthetic %d)\n", name, synth);
        digest(name, st, s);
        rt_scene_free(s);
    }
    // USD in each encoding (skinned, animated, a texture next to the layer or inside the package),
    // composed stages, and the error paths
    for (const char* name : {"seed.usda", "seed.usdc", "seed.usdz", "sub_over.usda", "ref_root.usda", "var_full.usda",
                             "composed.usdz", "truncated.usdc", "nolayer.usdz", "badjoint.usda", "missing.usda"}) {
        rt_scene* s = nullptr;
        rt_scene_new(&s);
        digest(name, rt_scene_add_usd(s, (in + "/" + name).c_str(), pos, rot, 0.5f, nullptr), s);
        rt_scene_free(s);
    }
    rt_scene* s = nullptr;
    rt_scene_new(&s);
    digest("seed.obj", rt_scene_add_obj(s, (in + "/seed.obj").c_str(), pos, rot, 2.0f, nullptr), s);
    digest("missing.obj", rt_scene_add_obj(s, "no/such/file.obj", zero, zero, 1.0f, nullptr), s);
    digest("procedural nonesuch", rt_scene_add_procedural(s, "nonesuch", nullptr, zero, zero, 1.0f, nullptr), s);
    uint32_t id = 0;
    digest("load_texture", rt_scene_load_texture(s, (in + "/seed.png").c_str(), &id), s);
    digest("load_texture missing", rt_scene_load_texture(s, "no/such.png", &id), s);
    digest("load_texture not a png", rt_scene_load_texture(s, (in + "/seed.obj").c_str(), &id), s);
    digest("bind_texture", rt_scene_bind_texture(s, 0, 0, 0, id), s);
    digest("bind_texture bad mesh", rt_scene_bind_texture(s, 99, 0, 0, 0), s);
    rt_scene_free(s);

    Camera cam;
    rt_camera_default(640, 360, &cam);
    Uniforms u;
    rt_uniforms_default(640, 360, 2, &u);
    std::vector<uint32_t> off(16 * 8);
    rt_random_offsets(42, 16, 8, off.data());
    std::printf("defaults\n");
    line("camera_default", &cam, sizeof cam);
    line("uniforms_default", &u, sizeof u);
    line("random_offsets(42,16,8)", off.data(), 4 * off.size());
    return 0;
}
