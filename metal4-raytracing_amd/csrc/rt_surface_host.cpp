// rt_surface_host.cpp — rt_debug_resolve_host: the surface query (rt_resolve_hits) over a scene
// description on the host.  It builds the arrays the kernel reads (the per-triangle normal
// records, the matrices, the materials, the texture tables) the way rt_scene_upload does and runs
// surface_eval (rt_surface.h), compiled for the host, over them.  No device call is made: the file
// also links into stand-alone host programs (tools/surface_host_check.cpp).
#include <exception>

#include "rt_scene_host.h"
#include "rt_surface.h"

using namespace rt;

extern "C" rt_status rt_debug_resolve_host(const rt_scene_desc* sd, const rt_ray* rays, const rt_ray_hit* hits, uint32_t n,
                                           rt_surface* surfaces, rt_surface_material* materials) {
    rt_ctx* const none = nullptr;
    if (!sd || (n && (!rays || !hits || !surfaces))) FAIL(none, RT_ERR_INVALID_ARG, "null argument");
    int max_sub = 1;
    uint64_t nv = 0, nt = 0;
    if (rt_status st = validate_scene(none, sd, max_sub, nv, nt)) return st;
    try {
        std::vector<float4> pos, nrm;
        std::vector<uint4> tri_info;
        std::vector<float> inst;
        flatten_scene(sd, pos, &nrm, tri_info, inst);
        // DevScene::tri_nrm as tri_nrm_k (rt_util.hip) writes it
        std::vector<float4> tri_nrm(4 * tri_info.size());
        for (size_t t = 0; t < tri_info.size(); ++t) {
            const uint4 ti = tri_info[t];
            const float4 n0 = nrm[ti.x], n1 = nrm[ti.y], n2 = nrm[ti.z];
            tri_nrm[4 * t + 0] = make_float4(n1.x, n1.y, n1.z, u2f(ti.w));
            tri_nrm[4 * t + 1] = make_float4(n2.x, n2.y, n2.z, 0.0f);
            tri_nrm[4 * t + 2] = make_float4(n0.x, n0.y, n0.z, 0.0f);
            tri_nrm[4 * t + 3] = __builtin_bit_cast(float4, ti);
        }
        Material zero_mat;
        std::memset(&zero_mat, 0, sizeof zero_mat);
        std::vector<Material> mat((size_t)max_sub * sd->mesh_count, zero_mat);
        for (uint32_t m = 0; m < sd->mesh_count; ++m)
            for (uint32_t s = 0; s < sd->meshes[m].submesh_count; ++s)
                mat[(size_t)m * max_sub + s] = sd->meshes[m].submeshes[s].material;
        TexTables T;
        build_tex_tables(sd, max_sub, (uint32_t)nv, T);
        DevScene S;
        std::memset(&S, 0, sizeof S);
        S.pos = pos.data();
        S.tri_nrm = tri_nrm.data();
        S.inst = inst.data();
        S.materials = mat.data();
        S.max_submeshes = max_sub;
        S.num_materials = (int)mat.size();
        S.num_tris = (int)nt;
        S.textured = T.textured ? 1 : 0;
        if (T.textured) {
            S.tex_texels = reinterpret_cast<const uchar4*>(T.texels.data());
            S.tex_info = T.info.data();
            S.mat_tex = T.mat_tex.data();
            S.uv = T.uv.data();
            S.tex_lut = T.lut;
        }
        for (uint32_t i = 0; i < n; ++i) {
            float4 w[4];
            std::memcpy(w, &rays[i], 32);
            std::memcpy(w + 2, &hits[i], 32);
            SurfaceWords r;
            const uint4 h1 = __builtin_bit_cast(uint4, w[3]);
            if (materials) {
                if (T.textured) surface_eval<true, true>(S, w[0], w[1], w[2], h1, r);
                else surface_eval<true, false>(S, w[0], w[1], w[2], h1, r);
                std::memcpy(&materials[i], &r.m0, 48);
            } else {
                if (T.textured) surface_eval<false, true>(S, w[0], w[1], w[2], h1, r);
                else surface_eval<false, false>(S, w[0], w[1], w[2], h1, r);
            }
            std::memcpy(&surfaces[i], &r.s0, 64);
        }
    } catch (const std::exception&) {   // nothing is thrown across the C-ABI
        FAIL(none, RT_ERR_OUT_OF_MEMORY, "rt_debug_resolve_host: allocation failed");
    }
    return RT_OK;
}
