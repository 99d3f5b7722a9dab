// rt_surface.h — the surface half of a hit: what raytracingKernel reads off the scene at the point
// a ray struck (Raytracing.metal:329-339, :391-456, :492-504), before anything is scattered.
//
// surface_point and shading_normal are the one text of it.  shade_step (rt_shade.h) calls them for
// the frame kernels with the matrix and the material of its LDS tables; surface_eval, below, calls
// them for a surface query (rq_resolve, rt_query.hip) and for the host hook
// (rt_debug_resolve_host) with the same records from global memory, and packs the result into the
// rt_surface / rt_surface_material records of include/rt_api.h.  Same function, same operands:
// the floats are equal bit for bit by construction, and what tests/test_gpu_surface.py pins
// through the G-buffer is the seam (the LDS tables against the global ones, the record packing).
#pragma once
#include "../../include/rt_api.h"
#include "rt_device.h"

namespace rt {

__host__ __device__ __forceinline__ uint32_t f2u(float x) { return __builtin_bit_cast(uint32_t, x); }
__host__ __device__ __forceinline__ float u2f(uint32_t x) { return __builtin_bit_cast(float, x); }
__host__ __device__ __forceinline__ f3 ldf3(const rt_float3& v) { return mk3(v.x, v.y, v.z); }
__host__ __device__ __forceinline__ f2 ld2(const float2& v) { return f2{v.x, v.y}; }

// The fields of a Material the kernel reads (Raytracing.metal:399-453), packed for LDS:
// base = (baseColor, opacity), emis = (emission, refractionIndex).
struct MatRec {
    float4 base;
    float4 emis;
};

// ---- texture path --------------------------------------------------------
// The reference samples with sampler(linear, linear, mip linear, address::repeat) in a compute
// kernel, i.e. bilinear from LOD 0 (Raytracing.metal:420).  Here: texel centres at integer + 0.5,
// wrap-around neighbours, each corner decoded through the byte table (sRGB for base color and
// emission maps, linear otherwise; alpha always linear), weights applied in a fixed order.
__host__ __device__ __forceinline__ float4 tex_sample(const DevScene& S, int t, f2 uv, bool srgb) {
    const uint4 ti = S.tex_info[t];
    const int w = (int)ti.y, h = (int)ti.z;
    float x = uv.x * (float)w - 0.5f, y = uv.y * (float)h - 0.5f;
    if (!(fabsf(x) < 1.0e9f)) x = 0.0f;   // NaN / huge coordinates
    if (!(fabsf(y) < 1.0e9f)) y = 0.0f;
    const float fx = floorf(x), fy = floorf(y);
    const float ax = x - fx, ay = y - fy, bx = 1.0f - ax, by = 1.0f - ay;
    int x0 = (int)((long long)fx % w), y0 = (int)((long long)fy % h);
    if (x0 < 0) x0 += w;
    if (y0 < 0) y0 += h;
    const int x1 = x0 + 1 == w ? 0 : x0 + 1, y1 = y0 + 1 == h ? 0 : y0 + 1;
    const uchar4* T = S.tex_texels + ti.x;
    const uchar4 c00 = T[(size_t)y0 * w + x0], c10 = T[(size_t)y0 * w + x1];
    const uchar4 c01 = T[(size_t)y1 * w + x0], c11 = T[(size_t)y1 * w + x1];
    const float* L = S.tex_lut;
    const float* Lc = L + (srgb ? 256 : 0);
    auto bil = [&](const float* lut, unsigned a, unsigned b, unsigned c, unsigned d) {
        return (lut[a] * bx + lut[b] * ax) * by + (lut[c] * bx + lut[d] * ax) * ay;
    };
    return make_float4(bil(Lc, c00.x, c10.x, c01.x, c11.x), bil(Lc, c00.y, c10.y, c01.y, c11.y),
                       bil(Lc, c00.z, c10.z, c01.z, c11.z), bil(L, c00.w, c10.w, c01.w, c11.w));
}

// computeTangentBasis (Raytracing.metal:185-218): object-space dP/du, dP/dv of the hit triangle
// from its vertices in the order (indices[3t+1], indices[3t+2], indices[3t]).
__host__ __device__ __forceinline__ bool tangent_basis(const DevScene& S, const uint4& ti, f3& tangent, f3& bitangent) {
    const f3 p0 = ld3(S.pos[ti.y]), p1 = ld3(S.pos[ti.z]), p2 = ld3(S.pos[ti.x]);
    const f2 uv0 = ld2(S.uv[ti.y]), uv1 = ld2(S.uv[ti.z]), uv2 = ld2(S.uv[ti.x]);
    const f3 e1 = p1 - p0, e2 = p2 - p0;
    const float d1x = uv1.x - uv0.x, d1y = uv1.y - uv0.y, d2x = uv2.x - uv0.x, d2y = uv2.y - uv0.y;
    const float denom = d1x * d2y - d1y * d2x;
    if (fabsf(denom) < 1e-8f) return false;
    const float r = 1.0f / denom;
    tangent = (e1 * d2y - e2 * d1y) * r;
    bitangent = (e2 * d1x - e1 * d2x) * r;
    return length(tangent) > 1e-8f && length(bitangent) > 1e-8f;
}

// What the scatter half (rt_scatter.h) and the callers read of a hit.  opacity is clamped to
// [0, 1]; ior is the material's refractionIndex as stored.  The map fields are what the
// debug-visualisation block and shading_normal go on with: tflags = 0 means no map is bound, and
// then tc is (0, 0), base is white and ti was not read.
struct SurfacePoint {
    f3 P, Ng, albedo, emission;
    float opacity, ior, roughness, metallic;
    unsigned tflags;   // the submesh's MATERIAL_TEXTURE_* bits
    int tnormal;       // its normal map
    f2 tc;
    float4 base;       // the base-colour sample
    uint4 ti;          // the triangle's vertex ids: the UVs and the tangent basis
};

// Raytracing.metal:336, :391-456.  rec is the triangle's tri_nrm line, (n1 | ti.w, n2, n0, ti),
// of which the caller has loaded rn1, rn2 and rn0 (it needs rn1.w to find M, the instance's 4x3,
// mat and slot); the fourth word is read only where a map is bound.  t, bu and bv are the hit's.
// MATERIAL = false skips the base-colour, roughness, metallic and emission samples (the caller
// passes constants in mat); TEXTURED = false compiles the sampler out.
template <bool MATERIAL, bool TEXTURED>
__host__ __device__ __forceinline__ void surface_point(const DevScene& S, const float4* rec, const float4 rn1,
                                                       const float4 rn2, const float4 rn0, const float* M,
                                                       const MatRec& mat, int slot, f3 rayO, f3 rayD, float t, float bu,
                                                       float bv, SurfacePoint& s) {
    const float bw = (1.0f - bu) - bv;                                                // :63-65
    s.P = rayO + rayD * t;                                                            // :336
    const f3 objN = (bu * ld3(rn1) + bv * ld3(rn2)) + bw * ld3(rn0);                  // :391
    s.Ng = normalize(xform(M, objN, 0.0f));                                           // :392-393
    if (length_lt_1e10(objN)) s.Ng = -rayD;                                           // :395-397

    s.albedo = ld3(mat.base);                                                         // :399
    s.roughness = 1.0f;                                                               // :431-441
    s.metallic = 0.0f;
    s.opacity = clampf(mat.base.w, 0.0f, 1.0f);                                       // :448
    s.emission = ld3(mat.emis);                                                       // :453
    s.ior = mat.emis.w;
    s.tflags = 0;
    s.tnormal = -1;
    s.tc = f2{0.0f, 0.0f};
    s.base = make_float4(1.0f, 1.0f, 1.0f, 1.0f);
    s.ti = make_uint4(0u, 0u, 0u, 0u);
    if (TEXTURED && S.textured) {                                                     // :400-456
        const int4 t0 = S.mat_tex[2 * slot], t1 = S.mat_tex[2 * slot + 1];
        s.tflags = (unsigned)t0.x;
        s.tnormal = t0.z;
        if (s.tflags) {                                                               // :412-417
            s.ti = __builtin_bit_cast(uint4, rec[3]);
            const f2 a = ld2(S.uv[s.ti.y]), b = ld2(S.uv[s.ti.z]), c = ld2(S.uv[s.ti.x]);
            s.tc.x = (bu * a.x + bv * b.x) + bw * c.x;
            s.tc.y = (bu * a.y + bv * b.y) + bw * c.y;
            s.tc.y = 1.0f - s.tc.y;
        }
        if (MATERIAL && (s.tflags & MATERIAL_TEXTURE_BASECOLOR)) {                    // :423-428
            s.base = tex_sample(S, t0.y, s.tc, true);
            s.albedo = s.albedo * mk3(s.base.x, s.base.y, s.base.z);
        }
        if (MATERIAL && (s.tflags & MATERIAL_TEXTURE_ROUGHNESS)) s.roughness = tex_sample(S, t0.w, s.tc, false).x;   // :431-434
        if (MATERIAL && (s.tflags & MATERIAL_TEXTURE_METALLIC)) s.metallic = tex_sample(S, t1.x, s.tc, false).x;     // :436-439
        if (s.tflags & MATERIAL_TEXTURE_OPACITY) s.opacity = s.opacity * tex_sample(S, t1.w, s.tc, false).x;         // :448-451
        if (MATERIAL && (s.tflags & MATERIAL_TEXTURE_EMISSION)) {                     // :453-456
            const float4 e = tex_sample(S, t1.z, s.tc, true);
            s.emission = mk3(e.x, e.y, e.z);
        }
    }
}

// The shading normal (Raytracing.metal:492-504): Ng, or the normal map's through the triangle's
// tangent frame.  Returns whether the map was applied.
template <bool TEXTURED>
__host__ __device__ __forceinline__ bool shading_normal(const DevScene& S, const SurfacePoint& s, const float* M,
                                                        f3& shadingNormal) {
    shadingNormal = s.Ng;                                                             // :492
    if (!(TEXTURED && (s.tflags & MATERIAL_TEXTURE_NORMAL))) return false;            // :493-504
    f3 tangent, bitangent;
    if (!tangent_basis(S, s.ti, tangent, bitangent)) return false;
    f3 worldT = xform(M, tangent, 0.0f);
    worldT = normalize(worldT - s.Ng * dot(worldT, s.Ng));
    const f3 worldB = normalize(cross(s.Ng, worldT));
    const float4 nm = tex_sample(S, s.tnormal, s.tc, false);
    const f3 n = mk3(nm.x * 2.0f - 1.0f, nm.y * 2.0f - 1.0f, nm.z * 2.0f - 1.0f);
    shadingNormal = normalize((n.x * worldT + n.y * worldB) + n.z * s.Ng);
    return true;
}

// The records as 16-B words: four of the surface, three of the material.
struct SurfaceWords {
    float4 s0, s1, s2;
    uint4 s3;
    float4 m0, m1, m2;
};

// One record of rt_resolve_hits.  o4 / d4: the ray's two words; h0 / h1: the hit's (t, u, v,
// triangle), (mesh, submesh, primitive, 0).  t, u and v are used as given.  The triangle id is the
// only index taken from the caller: anything at or above the scene's triangle count (RT_MISS
// included) is a miss and indexes nothing; the instance and the submesh that the matrix and the
// material are looked up by come from the library's own tri_nrm record.  MATERIAL = false leaves
// m0..m2 alone and reads neither the base colour nor the emission; the opacity and the refraction
// index are read either way, RT_SURFACE_TRANSMISSIVE needs them.  The caller passes
// TEXTURED = (S.textured != 0).
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
    const float4* const rec = S.tri_nrm + 4 * (size_t)id;
    const float4 rn1 = rec[0], rn2 = rec[1], rn0 = rec[2];
    const uint32_t tw = f2u(rn1.w);   // instance << 8 | submesh
    const float* M = S.inst + 12 * (size_t)(tw >> 8);
    const int slot = (int)(tw >> 8) * S.max_submeshes + (int)(tw & 0xffu);
    const float4* const mrec = reinterpret_cast<const float4*>(S.materials + slot);    // 64 B: four words
    const float4 mlast = mrec[3];   // (specularExponent, refractionIndex, opacity, textureFlags)
    MatRec mat{make_float4(1.0f, 1.0f, 1.0f, mlast.z), make_float4(0.0f, 0.0f, 0.0f, mlast.y)};
    if (MATERIAL) {
        const float4 b = mrec[0], e = mrec[2];
        mat.base = make_float4(b.x, b.y, b.z, mlast.z);
        mat.emis = make_float4(e.x, e.y, e.z, mlast.y);
    }
    const f3 rayD = ld3(d4);
    SurfacePoint s;
    surface_point<MATERIAL, TEXTURED>(S, rec, rn1, rn2, rn0, M, mat, slot, ld3(o4), rayD, h0.x, h0.y, h0.z, s);
    f3 shadingNormal;
    uint32_t flags = s.tflags ? RT_SURFACE_HAS_UV : 0u;
    if (shading_normal<TEXTURED>(S, s, M, shadingNormal)) flags |= RT_SURFACE_NORMAL_MAPPED;
    const float clampedOpacity = clampf(s.opacity, 0.0f, 1.0f);                        // :517
    const float ior = fmaxf(s.ior, 1.0f);
    if (clampedOpacity < 0.999f || ior > 1.01f) flags |= RT_SURFACE_TRANSMISSIVE;
    if (dot(rayD, s.Ng) > 0.0f) flags |= RT_SURFACE_BACKFACE;

    r.s0 = make_float4(s.P.x, s.P.y, s.P.z, h0.x);
    r.s1 = make_float4(s.Ng.x, s.Ng.y, s.Ng.z, s.tc.x);
    r.s2 = make_float4(shadingNormal.x, shadingNormal.y, shadingNormal.z, s.tc.y);
    r.s3 = make_uint4(id, h1.x, h1.y, flags);
    if (MATERIAL) {
        r.m0 = make_float4(s.albedo.x, s.albedo.y, s.albedo.z, clampedOpacity);
        r.m1 = make_float4(s.emission.x, s.emission.y, s.emission.z, ior);
        r.m2 = make_float4(s.roughness, s.metallic, mlast.w, u2f((uint32_t)slot));
    }
}

}  // namespace rt
