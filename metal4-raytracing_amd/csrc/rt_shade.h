// rt_shade.h — one hit-processing step of a path in a frame kernel: everything raytracingKernel
// does between two intersector calls (Raytracing.metal:324-774).  Shared by the per-pixel
// megakernel and the wavefront `shade` stage so both pipelines evaluate exactly the same operation
// sequence.
//
// Given the current ray and its closest hit, shade_step updates the path registers (throughput
// `color`, `accum`, bounce / step / transparencyPasses), optionally emits a shadow ray whose
// contribution the caller adds to `accum` when it is unoccluded (Raytracing.metal:741-743 /
// :667-669; a shadow ray whose contribution is ±0 is reported as `dark` instead and not traced:
// shadow_is_dark, rt_scatter.h), and either rewrites the ray for the next iteration (next = true)
// or ends the path.
// The arithmetic is not stated here: shade_step fetches the hit's records from the block's LDS
// tables (ShadeTabs), calls the surface half (surface_point / shading_normal, rt_surface.h) and
// the scatter half (scatter_step, rt_scatter.h), the functions the device queries and the host
// hooks call too, and keeps what only a frame has: the depth / motion outputs, the
// debug-visualisation modes and the G-buffer.  Also here: the primary ray and the pixel resolve.
#pragma once
#include "rt_kernels.h"
#include "rt_scatter.h"

namespace rt {

constexpr int kMatLds = 128;   // material records staged in LDS per block (4 KB)
constexpr int kInstLds = 32;   // instance matrices staged in LDS per block (48 B each, 1.5 KB)
constexpr int kLightLds = 8;   // lights staged in LDS per block (128 B each, 1 KB)

// Per-block lookup tables of the shading code: the first Halton dimensions, the scene's
// material records, instance matrices and lights in LDS (global memory beyond what was staged).
// A hit's instance matrix is the third load of a dependent chain (queue entry -> tri_nrm ->
// matrix) and its light record waits on the Halton light choice; from LDS each costs an LDS round
// trip instead of an L2 one (wf_shade 0.336 -> 0.310 ms per launch).
struct ShadeTabs {
    const HaltonDim* lds;
    const HaltonDim* glob;
    const MatRec* mat_lds;
    const Material* mat_glob;
    int n_mat_lds;             // = number of materials when they fit in LDS, else 0
    const float4* inst_lds;    // 3 float4 per instance: the 12 floats of its packed 4x3
    const float* inst_glob;
    int n_inst_lds;            // = number of instances when they fit in LDS, else 0
    const Light* light_lds;
    const Light* light_glob;
    int n_light_lds;           // = lightCount when the lights fit in LDS, else 0
    const SpotCone* spot_lds;  // spot_cone of every staged spotlight (load_tabs), beside its record
    int n_spot_lds;            // = n_light_lds when the caller gave load_tabs an array for them, else 0
    __device__ __forceinline__ float operator()(int i, int d) const {
        if (d == 0) return halton_base2(i);   // base 2: closed form (bit-identical, rt_math.h)
        return halton_fast(i, d < kHaltonLds ? lds[d] : glob[d]);
    }
    // scatter_step's draw policy of the frames (with light() below): the Halton number of the draw's dimension
    __device__ __forceinline__ float draw(Draw d, int i, int step) const { return (*this)(i, (int)draw_dim(d, step)); }
    __device__ __forceinline__ MatRec material(int slot) const {
        if (slot < n_mat_lds) return mat_lds[slot];
        const Material& m = mat_glob[slot];
        MatRec r;
        r.base = make_float4(m.baseColor.x, m.baseColor.y, m.baseColor.z, m.opacity);
        r.emis = make_float4(m.emission.x, m.emission.y, m.emission.z, m.refractionIndex);
        return r;
    }
    // The instance's 12 floats and the light record, from LDS when staged: one pointer that may
    // point to either (flat loads), which measured faster than a branch between an LDS and a
    // global load of the same record (wf_shade 0.310 vs 0.313 ms; both branches' registers)
    __device__ __forceinline__ const float* instance(int k) const {
        return k < n_inst_lds ? reinterpret_cast<const float*>(inst_lds + 3 * k) : inst_glob + 12 * (size_t)k;
    }
    __device__ __forceinline__ const Light& light(int k) const { return k < n_light_lds ? light_lds[k] : light_glob[k]; }
    // The spotlight's cone axis and cosine: ~80 VALU with an IEEE divide and a square root, and
    // pure functions of the record, so a staged light has them from load_tabs (once per block, not
    // once per hit that picks it); a light that is not staged computes them here, as before.
    __device__ __forceinline__ SpotCone spot(int k, const Light& l) const { return k < n_spot_lds ? spot_lds[k] : spot_cone(l); }
};

// Stages the Halton dimensions and the material records, instance matrices and lights of the
// scene in LDS (each table only when its LDS array is given and the scene's table fits; with
// lds_spot, also the spot_cone of each staged spotlight); every thread of the block calls it (ends
// with a barrier).
__device__ __forceinline__ ShadeTabs load_tabs(const DevScene& S, HaltonDim* lds_halton, MatRec* lds_mat,
                                               float4* lds_inst = nullptr, Light* lds_light = nullptr,
                                               SpotCone* lds_spot = nullptr, int light_count = 0) {
    for (int i = threadIdx.x; i < kHaltonLds; i += blockDim.x) lds_halton[i] = S.halton[i];
    const int n_mat = (lds_mat && S.num_materials <= kMatLds) ? S.num_materials : 0;
    for (int i = threadIdx.x; i < n_mat; i += blockDim.x) {
        const Material& m = S.materials[i];
        lds_mat[i].base = make_float4(m.baseColor.x, m.baseColor.y, m.baseColor.z, m.opacity);
        lds_mat[i].emis = make_float4(m.emission.x, m.emission.y, m.emission.z, m.refractionIndex);
    }
    const int n_inst_all = S.max_submeshes > 0 ? S.num_materials / S.max_submeshes : 0;
    const int n_inst = (lds_inst && n_inst_all <= kInstLds) ? n_inst_all : 0;
    const float4* ig = reinterpret_cast<const float4*>(S.inst);
    for (int i = threadIdx.x; i < 3 * n_inst; i += blockDim.x) lds_inst[i] = ig[i];
    const int n_light = (lds_light && light_count <= kLightLds) ? light_count : 0;
    for (int i = threadIdx.x; i < n_light; i += blockDim.x) {
        const Light l = S.lights[i];
        lds_light[i] = l;
        if (lds_spot && l.type == LightTypeSpotlight) lds_spot[i] = spot_cone(l);   // read for spotlights only
    }
    __syncthreads();
    return ShadeTabs{lds_halton, S.halton, lds_mat, S.materials, n_mat, lds_inst, S.inst, n_inst,
                     lds_light, S.lights, n_light, lds_spot, lds_spot ? n_light : 0};
}

struct StepResult {
    bool next;             // trace rayO/rayD again
    bool shadow;           // trace shadow ray; add contrib to accum when unoccluded
    bool dark;             // the step made a shadow ray that is not to be traced (shadow_is_dark): shadow is
                           // clear and the path goes on as after an occluded one; it still counts as a shadow ray
    f3 so, sd, contrib;
    float stmax;
    bool primary;          // bounce 0 / sample 0 hit: depth + motion (:342-389)
    float depth;
    f2 motion;
    bool gbuf;             // first hit of sample 0 with the G-buffer enabled (:506-515)
    float4 g0, g1, g2, g3;
};

__host__ __device__ __forceinline__ bool needs_full(const Uniforms& U, const DevScene& S) {
    return U.debugTextureMode != DebugTextureModeNone || U.enableDenoiseGBuffer != 0 || S.textured != 0;
}

// Depth and motion vector of a bounce-0 hit of sample 0 (Raytracing.metal:342-389): the hit
// point through this frame's and the previous frame's instance transforms and cameras.  Inline in
// the per-pixel kernel; the wavefront kernels record the hit and wf_motion evaluates this once
// per pixel after the pass (the last bounce-0 hit of sample 0 wins either way).  This function,
// extra_samples and resolve_pixel below are also, compiled for the host, the arithmetic of the
// temporal test hooks (rt_paths.h, rt_paths_host.cpp): S then carries tri_info, pos / prev_pos and
// inst / prev_inst only, as host pointers.
__host__ __device__ __forceinline__ void primary_outputs(const DevScene& S, const Uniforms& U, uint32_t id, float bu, float bv,
                                                float& depth_out, f2& motion_out) {
    const uint4 ti = S.tri_info[id];
    const int instanceIndex = (int)(ti.w >> 8);
    const float* M = S.inst + 12 * instanceIndex;
    const float bw = (1.0f - bu) - bv;
    const Camera& cam = U.camera;
    const f3 cright = ldf3(cam.right), cup = ldf3(cam.up), cfwd = ldf3(cam.forward);
    f3 op = (bu * ld3(S.pos[ti.y]) + bv * ld3(S.pos[ti.z])) + bw * ld3(S.pos[ti.x]);
    f3 pp = (bu * ld3(S.prev_pos[ti.y]) + bv * ld3(S.prev_pos[ti.z])) + bw * ld3(S.prev_pos[ti.x]);
    f3 worldPos = xform(M, op, 1.0f);
    f3 prevWorldPos = xform(S.prev_inst + 12 * instanceIndex, pp, 1.0f);
    f3 viewPos = worldPos - ldf3(cam.position);
    float sx = dot(viewPos, cright), sy = dot(viewPos, cup);
    float depth = dot(viewPos, cfwd);
    depth_out = fmaxf(depth, 1.0e-3f);
    float dd = fmaxf(depth, 0.001f);
    sx = sx / dd;
    sy = sy / dd;
    const Camera& pc = U.previousCamera;
    f3 pv = prevWorldPos - ldf3(pc.position);
    float psx = dot(pv, ldf3(pc.right)), psy = dot(pv, ldf3(pc.up));
    float pd = fmaxf(dot(pv, ldf3(pc.forward)), 0.001f);
    psx = psx / pd;
    psy = psy / pd;
    float mnx = sx - psx, mny = sy - psy;
    float rightScale = fmaxf(length(cright), 1e-5f);
    float upScale = fmaxf(length(cup), 1e-5f);
    float mpx = mnx * ((float)U.width / (2.0f * rightScale));
    float mpy = mny * ((float)U.height / (2.0f * upScale));
    motion_out.x = mpx;
    motion_out.y = -mpy;
}

// prevMotion / hadPrimaryHit / motionVector: only read by DebugTextureModeMotion.
// FULL = false compiles out the texture maps, the debug-visualisation and the G-buffer branches
// (the caller selects FULL = true whenever the scene is textured, uniforms.debugTextureMode != 0
// or enableDenoiseGBuffer != 0).
template <bool FULL, bool INLINE_PRIMARY = true>
__device__ __forceinline__ void shade_step(const DevScene& S, const Uniforms& U, const ShadeTabs& tabs, int hidx,
                                           int sampleIndex, f3& rayO, f3& rayD, const Hit& h, PathRegs& p,
                                           bool gbuf_pending, f2 prevMotion, bool hadPrimaryHit, f2 motionVector,
                                           StepResult& r) {
    r.next = false;
    r.shadow = false;
    r.dark = false;
    r.primary = false;
    r.gbuf = false;
    const float4* const rec = S.tri_nrm + 4 * (size_t)h.id;   // (n1 | ti.w, n2, n0, ti)
    const float4 rn1 = rec[0], rn2 = rec[1], rn0 = rec[2];
    const uint32_t tw = f2u(rn1.w);
    const int instanceIndex = (int)(tw >> 8), geometryIndex = (int)(tw & 0xffu);
    const int slot = instanceIndex * S.max_submeshes + geometryIndex;                 // :337-339
    const float* M = tabs.instance(instanceIndex);                                    // :329-333 (LDS)

    SurfacePoint s;                                                                   // :336, :391-456
    surface_point<true, FULL>(S, rec, rn1, rn2, rn0, M, tabs.material(slot), slot, rayO, rayD, h.t, h.u, h.v, s);

    if (p.bounce == 0 && sampleIndex == 0) {                                          // :342-389
        if (INLINE_PRIMARY) primary_outputs(S, U, h.id, h.u, h.v, r.depth, r.motion);
        r.primary = true;   // deferred: the caller records the hit for wf_motion
    }

    if (FULL && U.debugTextureMode != DebugTextureModeNone) {                         // :459-490
        f3 dc = mk3(0.0f, 0.0f, 0.0f);
        int m = U.debugTextureMode;
        if (m == DebugTextureModeBaseColor)
            dc = (s.tflags & MATERIAL_TEXTURE_BASECOLOR) ? mk3(s.base.x, s.base.y, s.base.z) : mk3(1.0f, 0.0f, 1.0f);
        else if (m == DebugTextureModeNormal) {
            if (s.tflags & MATERIAL_TEXTURE_NORMAL) {
                const float4 nm = tex_sample(S, s.tnormal, s.tc, false);
                dc = mk3(nm.x, nm.y, nm.z);
            } else {
                dc = s.Ng * 0.5f + mk3(0.5f, 0.5f, 0.5f);
            }
        }
        else if (m == DebugTextureModeRoughness) dc = mk3(s.roughness, s.roughness, s.roughness);
        else if (m == DebugTextureModeMetallic) dc = mk3(s.metallic, s.metallic, s.metallic);
        else if (m == DebugTextureModeAO) dc = mk3(1.0f, 0.0f, 1.0f);
        else if (m == DebugTextureModeEmission) dc = s.emission;
        else if (m == DebugTextureModeMotion) {
            f2 mp = r.primary ? r.motion : (hadPrimaryHit ? motionVector : prevMotion);
            float scx = clampf(mp.x * 0.05f, -1.0f, 1.0f), scy = clampf(mp.y * 0.05f, -1.0f, 1.0f);
            float mag = clampf(sqrtf(mp.x * mp.x + mp.y * mp.y) * 0.1f, 0.0f, 1.0f);
            dc = mk3(scx * 0.5f + 0.5f, scy * 0.5f + 0.5f, mag);
        }
        p.accum = dc;
        return;  // break
    }

    f3 shadingNormal;                                                                 // :492-504
    shading_normal<FULL>(S, s, M, shadingNormal);

    if (FULL && gbuf_pending && U.enableDenoiseGBuffer != 0 && sampleIndex == 0) {   // :506-515
        float rr = clampf(s.roughness, 0.0f, 1.0f);
        f3 da = s.albedo * (1.0f - s.metallic);
        f3 sa = mix3(mk3(0.04f, 0.04f, 0.04f), s.albedo, s.metallic);
        f3 on = shadingNormal * 0.5f + mk3(0.5f, 0.5f, 0.5f);
        r.g0 = make_float4(da.x, da.y, da.z, 1.0f);
        r.g1 = make_float4(sa.x, sa.y, sa.z, 1.0f);
        r.g2 = make_float4(on.x, on.y, on.z, 1.0f);
        r.g3 = make_float4(rr, 0.0f, 0.0f, 1.0f);
        r.gbuf = true;
    }

    r.next = scatter_step(tabs, U, hidx, s, shadingNormal, rayO, rayD, p, r.shadow, r.so, r.sd, r.stmax, r.contrib);   // :517-774
    // a contribution of ±0 leaves accum's bits alone whatever the ray finds (:741-743): not traced
    r.dark = r.shadow && shadow_is_dark(r.contrib);
    r.shadow = r.shadow && !r.dark;
}

// Primary ray for (pixel, sample) (Raytracing.metal:270-292).
__device__ __forceinline__ void primary_ray(const Uniforms& U, const ShadeTabs& halton, int px, int py, int hidx,
                                            f3& o, f3& d) {
    float rx = halton(hidx, 0), ry = halton(hidx, 1);
    float spx = (float)px + rx, spy = (float)py + ry;
    float uvx = spx / (float)U.width, uvy = spy / (float)U.height;
    uvx = uvx * 2.0f - 1.0f;
    uvy = uvy * 2.0f - 1.0f;
    const Camera& cam = U.camera;
    o = ldf3(cam.position);
    d = normalize((uvx * ldf3(cam.right) + uvy * ldf3(cam.up)) + ldf3(cam.forward));
}

// Motion-adaptive extra samples after sample 0 (Raytracing.metal:779-789).
__host__ __device__ __forceinline__ int extra_samples(const Uniforms& U, int maxExtra, f2 mv, f2 pm) {
    float motionMag = fmaxf(sqrtf(mv.x * mv.x + mv.y * mv.y), sqrtf(pm.x * pm.x + pm.y * pm.y));
    float low = fmaxf(U.motionSamplingLowThresholdPixels, 0.0f);
    float high = fmaxf(U.motionSamplingHighThresholdPixels, low + 1e-3f);
    float t = clampf((motionMag - low) / (high - low), 0.0f, 1.0f);
    int e = (int)roundf(t * (float)maxExtra);
    return min(max(e, 0), maxExtra);
}

// Average + temporal EMA (Raytracing.metal:792-817).
__host__ __device__ __forceinline__ f3 resolve_pixel(const Uniforms& U, f3 total, int totalSamples, f2 mv, f2 pm,
                                            const float4* accum_in, size_t pix) {
    total = total / (float)max(totalSamples, 1);
    if (U.frameIndex > 0) {
        float4 pc = accum_in[pix];
        f3 prevColor = mk3(pc.x, pc.y, pc.z);
        float historyWeight = clampf(U.accumulationWeight, 0.0f, 0.95f);
        if (U.enableMotionAdaptiveAccumulation != 0) {
            float motionMag = fmaxf(sqrtf(mv.x * mv.x + mv.y * mv.y), sqrtf(pm.x * pm.x + pm.y * pm.y));
            float low = fmaxf(U.motionAccumulationLowThresholdPixels, 0.0f);
            float high = fmaxf(U.motionAccumulationHighThresholdPixels, low + 1e-3f);
            float t = clampf((motionMag - low) / (high - low), 0.0f, 1.0f);
            float minWeight = clampf(U.motionAccumulationMinWeight, 0.0f, 0.95f);
            minWeight = fminf(minWeight, historyWeight);
            historyWeight = mixf(historyWeight, minWeight, t);
        }
        total = mix3(total, prevColor, historyWeight);
    }
    return total;
}

}  // namespace rt