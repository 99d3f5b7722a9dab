// rt_scatter.h — the scatter half of a hit: everything raytracingKernel does with a surface point
// once it has one (Raytracing.metal:517-774): glass, the light pick, the four light types, the
// legacy and GGX direct terms, the cosine bounce and the bounce / step bookkeeping.
//
// scatter_step is the one text of it.  shade_step (rt_shade.h) calls it for the frame kernels;
// scatter_eval, below, calls it for a shading query (rq_shade, rt_query.hip) and for the host hook
// (rt_debug_shade_host) on the records surface_eval (rt_surface.h) wrote.  The callers differ in
// two things only, which a draw policy answers: where random number D of step s of path i comes
// from, and where light record k lies.  Same function, same operands: the floats are equal bit
// for bit by construction, and what tests/test_gpu_shade.py pins through whole frames re-assembled
// from queries is the seam (the policies, the LDS tables against the global ones, the record
// packing).
#pragma once
#include "rt_surface.h"

namespace rt {

struct PathRegs {
    f3 color;
    f3 accum;
    int bounce, step, tpass;
};

// The six random numbers a step may draw, and the Halton dimension of each:
// 2 + step * stride + offset (Raytracing.metal:540, :588, :599-600, :763-764).  In unsigned
// arithmetic: a query's step is the caller's.
enum Draw { kDrawLight, kDrawAreaU, kDrawAreaV, kDrawGlass, kDrawBounce0, kDrawBounce1 };
RT_HD uint32_t draw_dim(Draw d, int step) {
    constexpr uint32_t stride[6] = {6u, 6u, 6u, 6u, 5u, 5u}, offset[6] = {0u, 1u, 2u, 5u, 3u, 4u};
    return 2u + (uint32_t)step * stride[d] + offset[d];
}

// min((int)(x * count), count - 1) of :588-589, with anything below 0 or NaN -> 0 and anything
// from count up -> count - 1 decided on the float: the same index for x in [0, 1), never one
// outside the lights for a caller's number.
RT_HD int scatter_light_index(float x, int count) {
    const float v = x * (float)count;
    if (!(v >= 0.0f)) return 0;
    return v < (float)count ? (int)v : count - 1;
}

// What a spotlight pick needs of its record besides position and colour (:608-632): the normalised
// cone axis and the cosine of the cone angle.  Pure functions of the record, so a draw policy may
// hand out values it computed once (ShadeTabs, rt_shade.h: per block, where the lights are staged)
// or compute them on the spot; either way by this one function, so the bits are the same.
struct SpotCone {
    f3 axis;
    float cos_angle;
};
RT_HD SpotCone spot_cone(const Light& light) {
    SpotCone c;
    c.axis = normalize(ldf3(light.direction));
    c.cos_angle = cos_pinned(light.coneAngle);
    return c;
}

// A shadow ray whose answer cannot change the image: its contribution is ±0 in every component
// (NdotL == 0 in PBR mode, which emits the ray whatever NdotL is, :692-744; or a zero colour
// product), and accum is never -0, so accum + contrib has accum's bits whether the ray is occluded
// or not.  False for NaN and for denormals.  The frame kernels do not trace such a ray
// (shade_step, rt_shade.h); the queries still hand it to the caller, by their record rules.
RT_HD bool shadow_is_dark(f3 contrib) { return contrib.x == 0.0f && contrib.y == 0.0f && contrib.z == 0.0f; }

// Raytracing.metal:517-774 at surface point s with shading normal shadingNormal.  rayO / rayD (in:
// the ray that hit; out: the next ray), color / accum, bounce / step / tpass are the renderer's
// registers.  draws.draw(D, i, step) is random number D of step `step` of Halton index i,
// draws.light(k) light record k, draws.spot(k, light) its spot_cone; U carries shadingMode,
// maxBounces and lightCount.  Sets shadow
// and the shadow ray (so, sd, stmax) with its contribution when the step emits one, and leaves
// them alone otherwise.  Returns whether the path goes on with rayO / rayD.
template <class DRAWS, class OPTS>
RT_HD bool scatter_step(const DRAWS& draws, const OPTS& U, int hidx, const SurfacePoint& s, f3 shadingNormal, f3& rayO,
                        f3& rayD, PathRegs& p, bool& shadow, f3& so, f3& sd, float& stmax, f3& contrib) {
    const float ao = 1.0f;                                                            // :443-446 (ENABLE_AO 0)
    float clampedOpacity = clampf(s.opacity, 0.0f, 1.0f);                            // :517-576
    float ior = fmaxf(s.ior, 1.0f);
    if (clampedOpacity < 0.999f || ior > 1.01f) {
        f3 N = shadingNormal, I = rayD;
        float cosi = clampf(dot(-I, N), -1.0f, 1.0f);
        float etaI = 1.0f, etaT = ior;
        if (cosi < 0.0f) {
            cosi = -cosi;
            N = -N;
            float tmp = etaI;
            etaI = etaT;
            etaT = tmp;
        }
        float eta = etaI / etaT;
        float k = 1.0f - (eta * eta) * (1.0f - cosi * cosi);
        float f0 = (etaT - etaI) / (etaT + etaI);
        f0 = f0 * f0;
        float F = f0 + (1.0f - f0) * pow5(clampf(1.0f - cosi, 0.0f, 1.0f));
        float transmission = 1.0f - clampedOpacity;
        float reflectWeight = F;
        float refractWeight = (1.0f - F) * transmission;
        float totalWeight = fmaxf(reflectWeight + refractWeight, 1e-4f);
        float reflectProb = reflectWeight / totalWeight;
        float choice = draws.draw(kDrawGlass, hidx, p.step);
        bool consumeBounce = true;
        if (k < 0.0f || choice < reflectProb) {
            f3 reflectDir = normalize(I - (2.0f * dot(I, N)) * N);
            rayO = s.P + reflectDir * 1e-3f;
            rayD = reflectDir;
            p.color = p.color * totalWeight;
        } else {
            float cosT = sqrtf(fmaxf(k, 0.0f));
            f3 refractDir = normalize(eta * I + (eta * cosi - cosT) * N);
            rayO = s.P + refractDir * 1e-3f;
            rayD = refractDir;
            p.color = p.color * (totalWeight * s.albedo);
            consumeBounce = false;
        }
        p.step++;
        if (consumeBounce) {
            p.bounce++;
            p.tpass = 0;
        } else {
            p.tpass++;
            if (p.tpass > U.maxBounces) {
                p.bounce++;
                p.tpass = 0;
            }
        }
        return p.bounce < U.maxBounces;
    }

    float perceptualRoughness = clampf(s.roughness, 0.04f, 1.0f);                     // :578-582
    float alpha = perceptualRoughness * perceptualRoughness;
    f3 diffuseColor = s.albedo;
    f3 F0 = mix3(mk3(0.04f, 0.04f, 0.04f), s.albedo, s.metallic);
    f3 V = normalize(-rayD);

    p.accum = p.accum + p.color * s.emission;                                         // :585

    float lightSample = draws.draw(kDrawLight, hidx, p.step);                         // :588-591
    const int lightIndex = scatter_light_index(lightSample, U.lightCount);
    const Light& light = draws.light(lightIndex);
    f3 Ldir, lightColor;
    float lightDistance;
    f3 lpos = ldf3(light.position), lcol = ldf3(light.color);
    if (light.type == LightTypeAreaLight) {                                           // :597-606, :95-129
        float ux = draws.draw(kDrawAreaU, hidx, p.step), uy = draws.draw(kDrawAreaV, hidx, p.step);
        ux = ux * 2.0f - 1.0f;
        uy = uy * 2.0f - 1.0f;
        f3 sp = (lpos + ldf3(light.right) * ux) + ldf3(light.up) * uy;
        Ldir = sp - s.P;
        lightDistance = length(Ldir);
        float inv = 1.0f / fmaxf(lightDistance, 1e-3f);
        Ldir = Ldir * inv;
        lightColor = lcol * (inv * inv);
        lightColor = lightColor * saturate(dot(-Ldir, ldf3(light.forward)));
    } else if (light.type == LightTypeSpotlight) {                                    // :608-632
        Ldir = lpos - s.P;
        lightDistance = length(Ldir);
        float inv = 1.0f / fmaxf(lightDistance, 1e-3f);
        Ldir = Ldir * inv;
        lightColor = mk3(0.0f, 0.0f, 0.0f);
        const SpotCone cone = draws.spot(lightIndex, light);   // normalize(direction), cos(coneAngle)
        float spotResult = dot(-Ldir, cone.axis);
        if (spotResult > cone.cos_angle) lightColor = (lcol * inv) * inv;
    } else if (light.type == LightTypePointlight) {                                   // :633-638
        Ldir = lpos - s.P;
        lightDistance = length(Ldir);
        float inv = 1.0f / fmaxf(lightDistance, 1e-3f);
        Ldir = Ldir * inv;
        lightColor = (lcol * inv) * inv;
    } else {                                                                          // :639-643
        Ldir = -normalize(ldf3(light.direction));
        lightDistance = INFINITY;
        lightColor = lcol;
    }
    lightColor = lightColor * (float)U.lightCount;                                    // :647
    f3 origin = s.P + s.Ng * 1e-3f;                                                   // :660, :683, :720, :769

    if (U.shadingMode == ShadingModeLegacy) {                                         // :649-690
        f3 L = normalize(Ldir);
        float NdotL = saturate(dot(shadingNormal, L));
        f3 legacyColor = p.color * s.albedo;
        if (length_lt_1e3(legacyColor)) return false;
        if (length_gt_1e4(lightColor) && NdotL > 0.0f) {
            shadow = true;
            so = origin;
            sd = Ldir;
            stmax = lightDistance - 1e-3f;
            contrib = (legacyColor * lightColor) * NdotL;
        }
        p.color = legacyColor * ao;
        if (length_lt_1e3(p.color)) return false;
    } else {
        if (length_gt_1e4(lightColor)) {                                              // :692-744
            f3 L = normalize(Ldir);
            f3 H = normalize(V + L);
            float NdotL = saturate(dot(shadingNormal, L));
            float NdotV = saturate(dot(shadingNormal, V));
            float NdotH = saturate(dot(shadingNormal, H));
            float VdotH = saturate(dot(V, H));
            f3 F = fresnelSchlick(VdotH, F0);
            float D = distributionGGX(NdotH, alpha);
            float kk = perceptualRoughness + 1.0f;
            kk = (kk * kk) / 8.0f;
            float G = geometrySmith(NdotV, NdotL, kk);
            f3 specular = ((D * G) * F) / fmaxf((4.0f * NdotV) * NdotL, 1e-4f);
            f3 kD = (mk3(1.0f, 1.0f, 1.0f) - F) * (1.0f - s.metallic);
            f3 diffuse = (kD * diffuseColor) / RT_PI;
            f3 direct = ((diffuse + specular) * lightColor) * NdotL;
            shadow = true;
            so = origin;
            sd = Ldir;
            stmax = lightDistance - 1e-3f;
            contrib = p.color * direct;
        }
        p.color = p.color * ((diffuseColor * (1.0f - s.metallic)) * ao);              // :748
        if (length_lt_1e3(p.color)) return false;                                     // :751-753
    }
    float r0 = draws.draw(kDrawBounce0, hidx, p.step), r1 = draws.draw(kDrawBounce1, hidx, p.step);   // :683-684, :763-764
    rayD = alignHemisphereWithNormal(sampleCosineWeightedHemisphere(r0, r1), shadingNormal);
    rayO = origin;                                                                    // :769-770
    p.step++;
    p.bounce++;
    p.tpass = 0;
    return p.bounce < U.maxBounces;
}

// ---- shading queries --------------------------------------------------------------------------

// rt_shade_opts with the light count resolved (0 = every uploaded light) and checked by the host.
struct ScatterOpts {
    int shadingMode, maxBounces, lightCount;
};

// The query's draw policy: the renderer's Halton numbers from the global table, or the caller's
// when RANDOMS, rnd0 = (light, area u, area v, glass choice), rnd1 = (r0, r1, -, -); the lights
// from global memory.  Every dimension drawn is >= 2, so the base-2 closed form of the frames'
// table (ShadeTabs, rt_shade.h) never applies.  The dimension is clamped to the table: a no-op for
// every state the renderer reaches (step <= 156, dimension <= 943), it keeps a caller's step from
// indexing outside the table.
template <bool RANDOMS>
struct QueryDraws {
    const HaltonDim* tab;
    const Light* lights;
    float4 rnd0, rnd1;
    __host__ __device__ __forceinline__ float draw(Draw d, int i, int step) const {
        if (RANDOMS) {
            switch (d) {
                case kDrawLight: return rnd0.x;
                case kDrawAreaU: return rnd0.y;
                case kDrawAreaV: return rnd0.z;
                case kDrawGlass: return rnd0.w;
                case kDrawBounce0: return rnd1.x;
                default: return rnd1.y;
            }
        }
        const uint32_t dim = draw_dim(d, step);
        return halton_fast(i, tab[dim < (uint32_t)RT_HALTON_DIMS ? dim : (uint32_t)(RT_HALTON_DIMS - 1)]);
    }
    __host__ __device__ __forceinline__ const Light& light(int k) const { return lights[k]; }
    __host__ __device__ __forceinline__ SpotCone spot(int, const Light& l) const { return spot_cone(l); }   // on the spot
};

// rt_path as 16-B words: (throughput, sample), (radiance, flags), (bounce, step, passes, reserved).
struct PathWords {
    float4 p0, p1;
    int4 p2;
};

// The three output records: next ray (origin, direction | tmax), shadow ray, contribution.
struct ScatterOut {
    float4 n0, n1, h0, h1, c;
};

// One record of rt_shade_hits.  d4: the traced ray's direction word; s0..s3 / m0..m2: its
// rt_surface and rt_surface_material; rnd0 / rnd1: the caller's numbers (RANDOMS).  Updates the
// path in place and fills the three output records by the record rules of include/rt_api.h: a
// path that is not shaded (ALIVE clear; or ALIVE with bounce >= maxBounces or a miss surface, the
// renderer's `while` / `break`) only has its ALIVE and SHADOW bits cleared, and whatever a step
// does not produce is zero-filled with tmax = -1.
template <bool RANDOMS>
RT_HD void scatter_eval(const HaltonDim* tab, const Light* lights, const ScatterOpts& U, const float4 d4, const float4 s0,
                        const float4 s1, const float4 s2, const uint4 s3, const float4 m0, const float4 m1,
                        const float4 m2, const float4 rnd0, const float4 rnd1, PathWords& w, ScatterOut& o) {
    o.n0 = o.h0 = o.c = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    o.n1 = o.h1 = make_float4(0.0f, 0.0f, 0.0f, -1.0f);
    const uint32_t flags_in = f2u(w.p1.w);
    uint32_t flags = flags_in & ~(RT_PATH_ALIVE | RT_PATH_SHADOW);
    if (!(flags_in & RT_PATH_ALIVE) || w.p2.x >= U.maxBounces || s3.x == RT_MISS) {
        w.p1.w = u2f(flags);
        return;
    }
    PathRegs p;
    p.color = ld3(w.p0);
    p.accum = ld3(w.p1);
    p.bounce = w.p2.x;
    p.step = w.p2.y;
    p.tpass = w.p2.z;
    SurfacePoint s;   // the fields scatter_step reads
    s.P = ld3(s0);
    s.Ng = ld3(s1);
    s.albedo = ld3(m0);
    s.opacity = m0.w;
    s.emission = ld3(m1);
    s.ior = m1.w;
    s.roughness = m2.x;
    s.metallic = m2.y;
    f3 rayO = mk3(0.0f, 0.0f, 0.0f), rayD = ld3(d4);
    bool shadow = false;
    f3 so = rayO, sd = rayO, contrib = rayO;
    float stmax = -1.0f;
    const QueryDraws<RANDOMS> draws{tab, lights, rnd0, rnd1};
    const bool next = scatter_step(draws, U, (int)f2u(w.p0.w), s, ld3(s2), rayO, rayD, p, shadow, so, sd, stmax, contrib);
    if (next) {
        flags |= RT_PATH_ALIVE;
        o.n0 = make_float4(rayO.x, rayO.y, rayO.z, 0.0f);
        o.n1 = make_float4(rayD.x, rayD.y, rayD.z, INFINITY);
    }
    if (shadow) {
        flags |= RT_PATH_SHADOW;
        o.h0 = make_float4(so.x, so.y, so.z, 0.0f);
        o.h1 = make_float4(sd.x, sd.y, sd.z, stmax);
        o.c = make_float4(contrib.x, contrib.y, contrib.z, 0.0f);
    }
    w.p0 = make_float4(p.color.x, p.color.y, p.color.z, w.p0.w);
    w.p1 = make_float4(p.accum.x, p.accum.y, p.accum.z, u2f(flags));
    w.p2 = make_int4(p.bounce, p.step, p.tpass, w.p2.w);
}

}  // namespace rt
