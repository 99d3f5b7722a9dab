// rt_surface.h — a ray-query hit resolved into what the renderer would shade there: the surface
// record (rt_surface) and the material record (rt_surface_material) of include/rt_api.h.
//
// surface_eval states the expressions of shade_step (rt_shade.h, :208-263 and :292-303 there) in
// the same order on the same operands, so every float equals the one a frame kernel forms at that
// hit bit for bit; tests/test_gpu_surface.py pins the two against each other through the G-buffer.
// shade_step itself does not call it: the frame kernels read their materials and matrices from LDS
// tables and their register counts are tuned (Makefile).  Compiled for gfx950 (rq_resolve,
// rt_query.hip) and for the host (rt_debug_resolve_host).
#pragma once
#include "../../include/rt_api.h"
#include "rt_shade.h"

namespace rt {

// The records as 16-B words: four of the surface, three of the material.
struct SurfaceWords {
    float4 s0, s1, s2;
    uint4 s3;
    float4 m0, m1, m2;
};

__host__ __device__ __forceinline__ uint32_t f2u(float x) { return __builtin_bit_cast(uint32_t, x); }
__host__ __device__ __forceinline__ float u2f(uint32_t x) { return __builtin_bit_cast(float, x); }

// o4 / d4: the ray's two words; h0 / h1: the hit's (t, u, v, triangle), (mesh, submesh, primitive, 0).
// t, u and v are used as given.  The triangle id is the only index taken from the caller: anything
// at or above the scene's triangle count (RT_MISS included) is a miss and indexes nothing; the
// instance and the submesh that the matrix and the material are looked up by come from the
// library's own tri_nrm record.  MATERIAL = false leaves m0..m2 alone and skips the base-colour,
// roughness, metallic and emission loads; the opacity and the refraction index are read either
// way, RT_SURFACE_TRANSMISSIVE needs them.  TEXTURED = false compiles the sampler out (the caller
// passes S.textured != 0).
template <bool MATERIAL, bool TEXTURED>
__host__ __device__ __forceinline__ void surface_eval(const DevScene& S, const float4 o4, const float4 d4, const float4 h0,
                                                      const uint4 h1, SurfaceWords& r) {
    const uint32_t id = f2u(h0.w);
    if (id >= (uint32_t)S.num_tris) {
        r.s0 = make_float4(0.0f, 0.0f, 0.0f, INFINITY);
        r.s1 = r.s2 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        r.s3 = make_uint4(RT_MISS, RT_MISS, RT_MISS, 0u);
        if (MATERIAL) r.m0 = r.m1 = r.m2 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        return;
    }
    const float4* const rec = S.tri_nrm + 4 * (size_t)id;   // (n1 | ti.w, n2, n0, ti)
    const float4 rn1 = rec[0], rn2 = rec[1], rn0 = rec[2];
    const uint32_t tw = f2u(rn1.w);
    const int instanceIndex = (int)(tw >> 8);
    const int geometryIndex = (int)(tw & 0xffu);
    const float* M = S.inst + 12 * (size_t)instanceIndex;                             // :329-333
    const f3 rayO = ld3(o4), rayD = ld3(d4);
    const f3 P_ = rayO + rayD * h0.x;                                                  // :336
    const int slot = instanceIndex * S.max_submeshes + geometryIndex;                  // :337-339
    const float4* const mrec = reinterpret_cast<const float4*>(S.materials + slot);    // 64 B: four words
    const float4 mlast = mrec[3];   // (specularExponent, refractionIndex, opacity, textureFlags)
    const float bu = h0.y, bv = h0.z, bw = (1.0f - bu) - bv;                           // :63-65

    const f3 objN = (bu * ld3(rn1) + bv * ld3(rn2)) + bw * ld3(rn0);                   // :391
    f3 Ng = normalize(xform(M, objN, 0.0f));                                           // :392-393
    if (length_lt_1e10(objN)) Ng = -rayD;                                              // :395-397

    f3 albedo = mk3(1.0f, 1.0f, 1.0f), emission = mk3(0.0f, 0.0f, 0.0f);
    if (MATERIAL) {
        albedo = ld3(mrec[0]);                                                         // :399
        emission = ld3(mrec[2]);                                                       // :453
    }
    float roughness = 1.0f, metallic = 0.0f;                                           // :431-441
    float opacity = clampf(mlast.z, 0.0f, 1.0f);                                       // :448
    unsigned tflags = 0;
    int tnormal = -1;
    f2 tc = f2{0.0f, 0.0f};
    uint4 ti = make_uint4(0u, 0u, 0u, tw);
    if (TEXTURED) {
        const int4 t0 = S.mat_tex[2 * slot], t1 = S.mat_tex[2 * slot + 1];
        tflags = (unsigned)t0.x;
        tnormal = t0.z;
        if (tflags) {                                                                  // :412-417
            ti = __builtin_bit_cast(uint4, rec[3]);   // vertex indices for the UVs and the tangent basis
            const f2 a = ld2(S.uv[ti.y]), b = ld2(S.uv[ti.z]), c = ld2(S.uv[ti.x]);
            tc.x = (bu * a.x + bv * b.x) + bw * c.x;
            tc.y = (bu * a.y + bv * b.y) + bw * c.y;
            tc.y = 1.0f - tc.y;
        }
        if (MATERIAL && (tflags & MATERIAL_TEXTURE_BASECOLOR)) {                       // :423-428
            const float4 bsample = tex_sample(S, t0.y, tc, true);
            albedo = albedo * mk3(bsample.x, bsample.y, bsample.z);
        }
        if (MATERIAL && (tflags & MATERIAL_TEXTURE_ROUGHNESS)) roughness = tex_sample(S, t0.w, tc, false).x;   // :431-434
        if (MATERIAL && (tflags & MATERIAL_TEXTURE_METALLIC)) metallic = tex_sample(S, t1.x, tc, false).x;     // :436-439
        if (tflags & MATERIAL_TEXTURE_OPACITY) opacity = opacity * tex_sample(S, t1.w, tc, false).x;           // :448-451
        if (MATERIAL && (tflags & MATERIAL_TEXTURE_EMISSION)) {                        // :453-456
            const float4 e = tex_sample(S, t1.z, tc, true);
            emission = mk3(e.x, e.y, e.z);
        }
    }

    uint32_t flags = tflags ? RT_SURFACE_HAS_UV : 0u;
    f3 shadingNormal = Ng;                                                             // :492
    if (TEXTURED && (tflags & MATERIAL_TEXTURE_NORMAL)) {                              // :493-504
        f3 tangent, bitangent;
        if (tangent_basis(S, ti, tangent, bitangent)) {
            f3 worldT = xform(M, tangent, 0.0f);
            worldT = normalize(worldT - Ng * dot(worldT, Ng));
            const f3 worldB = normalize(cross(Ng, worldT));
            const float4 nm = tex_sample(S, tnormal, tc, false);
            const f3 n = mk3(nm.x * 2.0f - 1.0f, nm.y * 2.0f - 1.0f, nm.z * 2.0f - 1.0f);
            shadingNormal = normalize((n.x * worldT + n.y * worldB) + n.z * Ng);
            flags |= RT_SURFACE_NORMAL_MAPPED;
        }
    }

    const float clampedOpacity = clampf(opacity, 0.0f, 1.0f);                          // :517
    const float ior = fmaxf(mlast.y, 1.0f);
    if (clampedOpacity < 0.999f || ior > 1.01f) flags |= RT_SURFACE_TRANSMISSIVE;
    if (dot(rayD, Ng) > 0.0f) flags |= RT_SURFACE_BACKFACE;

    r.s0 = make_float4(P_.x, P_.y, P_.z, h0.x);
    r.s1 = make_float4(Ng.x, Ng.y, Ng.z, tc.x);
    r.s2 = make_float4(shadingNormal.x, shadingNormal.y, shadingNormal.z, tc.y);
    r.s3 = make_uint4(id, h1.x, h1.y, flags);
    if (MATERIAL) {
        r.m0 = make_float4(albedo.x, albedo.y, albedo.z, clampedOpacity);
        r.m1 = make_float4(emission.x, emission.y, emission.z, ior);
        r.m2 = make_float4(roughness, metallic, mlast.w, u2f((uint32_t)slot));
    }
}

}  // namespace rt
