// rt_scatter.h — a shading query: one resolved hit and its path state turned into the path's next
// ray, its shadow ray and the updated state (rt_shade_hits, include/rt_api.h).
//
// scatter_step states the expressions of shade_step (rt_shade.h, :317-474 there: everything after
// the material fetch) in the same order on the same operands, so every float equals the one a
// frame kernel forms at that hit with the same path state, bit for bit.  Its inputs are the
// records surface_eval (rt_surface.h) wrote: P, Ng, the shading normal, the albedo, the clamped
// opacity, the emission, max(ior, 1), roughness and metallic.  shade_step itself does not call it
// (LDS tables, tuned register counts: see rt_surface.h); tests/test_gpu_shade.py pins the two
// against each other through whole frames re-assembled from queries.  Compiled for gfx950
// (rq_shade, rt_query.hip) and for the host (rt_debug_shade_host).
#pragma once
#include "rt_surface.h"

namespace rt {

// rt_shade_opts with the light count resolved (0 = every uploaded light) and checked by the host.
struct ScatterOpts {
    int shadingMode, maxBounces, lightCount;
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

// The renderer's Halton number (halton of rt_shade.h's ShadeTabs) from the global table.  Every
// dimension drawn here is >= 2, so the base-2 closed form never applies.  The dimension is
// clamped to the table: a no-op for every state the renderer reaches (step <= 156, dimension
// <= 943), it keeps a caller's step from indexing outside the table.
RT_HD float scatter_halton(const HaltonDim* tab, int i, int step, uint32_t stride, uint32_t k) {
    const uint32_t d = 2u + (uint32_t)step * stride + k;
    return halton_fast(i, tab[d < (uint32_t)RT_HALTON_DIMS ? d : (uint32_t)(RT_HALTON_DIMS - 1)]);
}

RT_HD f3 ld3l(const rt_float3& v) { return mk3(v.x, v.y, v.z); }   // rt_shade.h's ldf3, for the host too

// min((int)(x * count), count - 1) of :588-589, with anything below 0 or NaN -> 0 and anything
// from count up -> count - 1 decided on the float: the same index for x in [0, 1), never one
// outside the lights for a caller's number.
RT_HD int scatter_light_index(float x, int count) {
    const float v = x * (float)count;
    if (!(v >= 0.0f)) return 0;
    return v < (float)count ? (int)v : count - 1;
}

// shade_step from :317 on.  rayO / rayD, color / accum, bounce / step / tpass are the renderer's
// registers; rnd0 = (light, area u, area v, glass choice), rnd1 = (r0, r1, -, -) replace the
// Halton numbers when RANDOMS.  Returns shade_step's r.next.
template <bool RANDOMS>
RT_HD bool scatter_step(const HaltonDim* tab, const Light* lights, const ScatterOpts& U, int hidx, const float4 rnd0,
                        const float4 rnd1, f3 P_, f3 Ng, f3 shadingNormal, f3 albedo, float opacity, f3 emission,
                        float ior_in, float roughness, float metallic, f3& rayO, f3& rayD, PathRegs& p, bool& shadow,
                        f3& so, f3& sd, float& stmax, f3& contrib) {
    const float ao = 1.0f;                                                            // :443-446 (ENABLE_AO 0)
    float clampedOpacity = clampf(opacity, 0.0f, 1.0f);                              // :517-576
    float ior = fmaxf(ior_in, 1.0f);
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
        float choice = RANDOMS ? rnd0.w : scatter_halton(tab, hidx, p.step, 6u, 5u);
        bool consumeBounce = true;
        if (k < 0.0f || choice < reflectProb) {
            f3 reflectDir = normalize(I - (2.0f * dot(I, N)) * N);
            rayO = P_ + reflectDir * 1e-3f;
            rayD = reflectDir;
            p.color = p.color * totalWeight;
        } else {
            float cosT = sqrtf(fmaxf(k, 0.0f));
            f3 refractDir = normalize(eta * I + (eta * cosi - cosT) * N);
            rayO = P_ + refractDir * 1e-3f;
            rayD = refractDir;
            p.color = p.color * (totalWeight * albedo);
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

    float perceptualRoughness = clampf(roughness, 0.04f, 1.0f);                       // :578-582
    float alpha = perceptualRoughness * perceptualRoughness;
    f3 diffuseColor = albedo;
    f3 F0 = mix3(mk3(0.04f, 0.04f, 0.04f), albedo, metallic);
    f3 V = normalize(-rayD);

    p.accum = p.accum + p.color * emission;                                           // :585

    float lightSample = RANDOMS ? rnd0.x : scatter_halton(tab, hidx, p.step, 6u, 0u);   // :588-591
    int lightIndex = scatter_light_index(lightSample, U.lightCount);
    const Light& light = lights[lightIndex];
    f3 Ldir, lightColor;
    float lightDistance;
    f3 lpos = ld3l(light.position), lcol = ld3l(light.color);
    if (light.type == LightTypeAreaLight) {                                           // :597-606, :95-129
        float ux = RANDOMS ? rnd0.y : scatter_halton(tab, hidx, p.step, 6u, 1u);
        float uy = RANDOMS ? rnd0.z : scatter_halton(tab, hidx, p.step, 6u, 2u);
        ux = ux * 2.0f - 1.0f;
        uy = uy * 2.0f - 1.0f;
        f3 sp = (lpos + ld3l(light.right) * ux) + ld3l(light.up) * uy;
        Ldir = sp - P_;
        lightDistance = length(Ldir);
        float inv = 1.0f / fmaxf(lightDistance, 1e-3f);
        Ldir = Ldir * inv;
        lightColor = lcol * (inv * inv);
        lightColor = lightColor * saturate(dot(-Ldir, ld3l(light.forward)));
    } else if (light.type == LightTypeSpotlight) {                                    // :608-632
        Ldir = lpos - P_;
        lightDistance = length(Ldir);
        float inv = 1.0f / fmaxf(lightDistance, 1e-3f);
        Ldir = Ldir * inv;
        lightColor = mk3(0.0f, 0.0f, 0.0f);
        f3 coneDirection = normalize(ld3l(light.direction));
        float spotResult = dot(-Ldir, coneDirection);
        if (spotResult > cos_pinned(light.coneAngle)) lightColor = (lcol * inv) * inv;
    } else if (light.type == LightTypePointlight) {                                   // :633-638
        Ldir = lpos - P_;
        lightDistance = length(Ldir);
        float inv = 1.0f / fmaxf(lightDistance, 1e-3f);
        Ldir = Ldir * inv;
        lightColor = (lcol * inv) * inv;
    } else {                                                                          // :639-643
        Ldir = -normalize(ld3l(light.direction));
        lightDistance = INFINITY;
        lightColor = lcol;
    }
    lightColor = lightColor * (float)U.lightCount;                                    // :647
    f3 origin = P_ + Ng * 1e-3f;                                                      // :660, :683, :720, :769

    if (U.shadingMode == ShadingModeLegacy) {                                         // :649-690
        f3 L = normalize(Ldir);
        float NdotL = saturate(dot(shadingNormal, L));
        f3 legacyColor = p.color * albedo;
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
        float r0 = RANDOMS ? rnd1.x : scatter_halton(tab, hidx, p.step, 5u, 3u);
        float r1 = RANDOMS ? rnd1.y : scatter_halton(tab, hidx, p.step, 5u, 4u);
        rayD = alignHemisphereWithNormal(sampleCosineWeightedHemisphere(r0, r1), shadingNormal);
        rayO = origin;
        p.step++;
        p.bounce++;
        p.tpass = 0;
        return p.bounce < U.maxBounces;
    }

    if (length_gt_1e4(lightColor)) {                                                  // :692-744
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
        f3 kD = (mk3(1.0f, 1.0f, 1.0f) - F) * (1.0f - metallic);
        f3 diffuse = (kD * diffuseColor) / RT_PI;
        f3 direct = ((diffuse + specular) * lightColor) * NdotL;
        shadow = true;
        so = origin;
        sd = Ldir;
        stmax = lightDistance - 1e-3f;
        contrib = p.color * direct;
    }

    p.color = p.color * ((diffuseColor * (1.0f - metallic)) * ao);                    // :748
    if (length_lt_1e3(p.color)) return false;                                         // :751-753
    float r0 = RANDOMS ? rnd1.x : scatter_halton(tab, hidx, p.step, 5u, 3u);      // :763-764
    float r1 = RANDOMS ? rnd1.y : scatter_halton(tab, hidx, p.step, 5u, 4u);
    rayD = alignHemisphereWithNormal(sampleCosineWeightedHemisphere(r0, r1), shadingNormal);
    rayO = origin;                                                                    // :769-770
    p.step++;
    p.bounce++;
    p.tpass = 0;
    return p.bounce < U.maxBounces;
}

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
    f3 rayO = mk3(0.0f, 0.0f, 0.0f), rayD = ld3(d4);
    bool shadow = false;
    f3 so = rayO, sd = rayO, contrib = rayO;
    float stmax = -1.0f;
    const bool next = scatter_step<RANDOMS>(tab, lights, U, (int)f2u(w.p0.w), rnd0, rnd1, ld3(s0), ld3(s1), ld3(s2),
                                            ld3(m0), m0.w, ld3(m1), m1.w, m2.x, m2.y, rayO, rayD, p, shadow, so, sd,
                                            stmax, contrib);
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
