// rt_paths.h — the per-record code of the path queries (include/rt_api.h: rt_camera_paths,
// rt_connect_paths, rt_retire_paths, rt_average_samples) and the tile geometry of
// rt_compact_paths.  One text for the kernels (rq_camera .. rq_average, rt_query.hip) and the host
// hooks (rt_paths_host.cpp), as rt_scatter.h is for the shading query: same function, same
// operands, so the floats are equal bit for bit by construction.  Also the per-record code of the
// temporal hooks (rt_debug_primary_outputs_host, rt_debug_extra_paths_host,
// rt_debug_resolve_samples_host): record selection and layout around the frames' own arithmetic
// (rt_shade.h), written host / device like the rest; only the hooks call it so far.
#pragma once
#include "rt_shade.h"     // primary_outputs, extra_samples, resolve_pixel: the frames' own arithmetic
#include "rt_surface.h"   // ldf3, f2u / u2f

namespace rt {

// ---- camera paths ----------------------------------------------------------------------------------
// The most extra samples a pixel can take (Raytracing.metal:777-779): the stride of the Halton
// indices and of the temporal hooks' tags counts them whether a pixel takes them or not.
RT_HD int max_extra_samples(const Uniforms& U) {
    return (U.enableMotionAdaptiveSampling != 0 && U.motionSamplingMaxExtraSamples > 0) ? U.motionSamplingMaxExtraSamples : 0;
}

// Halton index of sample s of a pixel whose random offset is rnd: base_hidx of rt_wavefront.hip
// (Raytracing.metal:263-270) in unsigned arithmetic, the same bits.
RT_HD uint32_t camera_hidx(const Uniforms& U, uint32_t rnd, int s) {
    const int spp = U.samplesPerPixel > 1 ? U.samplesPerPixel : 1;
    return rnd + (U.frameIndex * ((uint32_t)spp + (uint32_t)max_extra_samples(U)) + (uint32_t)s);
}

// rt_ray and rt_path of a camera path as 16-B words.
struct CameraWords {
    float4 r0, r1;   // origin | 0, direction | tmax
    float4 p0, p1;   // throughput | sample, radiance | flags
    uint4 p2;        // bounce, step, passes, tag
};

// Record of pixel pix, sample s: primary_ray of rt_shade.h (Raytracing.metal:270-292) with the
// Halton numbers of dimensions 0 (closed form) and 1 (tab1 = the table's entry 1), and the path
// state Renderer.make_paths makes.
RT_HD void camera_record(const Uniforms& U, const HaltonDim& tab1, uint32_t rnd, uint32_t pix, int s, uint32_t tag,
                         CameraWords& w) {
    const int px = (int)(pix % (uint32_t)U.width), py = (int)(pix / (uint32_t)U.width);
    const uint32_t hidx = camera_hidx(U, rnd, s);
    const float rx = halton_base2((int)hidx), ry = halton_fast((int)hidx, tab1);
    const float spx = (float)px + rx, spy = (float)py + ry;
    float uvx = spx / (float)U.width, uvy = spy / (float)U.height;
    uvx = uvx * 2.0f - 1.0f;
    uvy = uvy * 2.0f - 1.0f;
    const Camera& cam = U.camera;
    const f3 o = ldf3(cam.position);
    const f3 d = normalize((uvx * ldf3(cam.right) + uvy * ldf3(cam.up)) + ldf3(cam.forward));
    w.r0 = make_float4(o.x, o.y, o.z, 0.0f);
    w.r1 = make_float4(d.x, d.y, d.z, INFINITY);
    w.p0 = make_float4(1.0f, 1.0f, 1.0f, u2f(hidx));
    w.p1 = make_float4(0.0f, 0.0f, 0.0f, u2f(RT_PATH_ALIVE));
    w.p2 = make_uint4(0u, 0u, 0u, tag);
}

// ---- connect / retire / average ----------------------------------------------------------------------
// radiance += contrib on the path's second word: the renderer's accum = accum + contrib
// (Raytracing.metal:741-743); the flags ride along unchanged.
RT_HD float4 connect_word(const float4 p1, const float4 c) {
    return make_float4(p1.x + c.x, p1.y + c.y, p1.z + c.z, p1.w);
}

// A retired path's sample: its radiance, alpha 1.
RT_HD float4 retire_word(const float4 p1) { return make_float4(p1.x, p1.y, p1.z, 1.0f); }

// The pixel of spp samples at s: summed in sample order, divided as resolve_pixel (rt_shade.h)
// divides for frame 0; alpha 1 as the frame kernels store it.
RT_HD float4 average_pixel(const float4* s, uint32_t spp) {
    f3 total = ld3(s[0]);
    for (uint32_t k = 1; k < spp; ++k) total = total + ld3(s[k]);
    total = total / (float)spp;
    return make_float4(total.x, total.y, total.z, 1.0f);
}

// ---- temporal hooks: depth / motion, extra samples, the EMA -------------------------------------------
// Which records rt_debug_primary_outputs_host uses, from the path's flags / bounce / tag words alone (read
// before anything else of the record): a live path at bounce 0 whose tag is sample `offset` of a
// pixel below `pixels`.  The renderer's `bounce == 0 && sampleIndex == 0` (Raytracing.metal:342).
RT_HD bool primary_selected(uint32_t flags, int bounce, uint32_t tag, uint32_t stride, uint32_t offset, uint32_t pixels,
                            uint32_t& pix) {
    if ((flags & RT_PATH_ALIVE) == 0u || bounce != 0) return false;
    pix = tag / stride;
    return tag - pix * stride == offset && pix < pixels;
}

// Depth and motion of a selected record's hit (h0: t, u, v, triangle): primary_outputs itself.
// False for a miss or a triangle the scene does not have; nothing is indexed then.
RT_HD bool primary_record(const DevScene& S, const Uniforms& U, const float4 h0, float& depth, f2& motion) {
    const uint32_t id = f2u(h0.w);
    if (id >= (uint32_t)S.num_tris) return false;
    primary_outputs(S, U, id, h0.y, h0.z, depth, motion);
    return true;
}

// Two floats of a motion target as f2; a null target reads as zeros (the targets after rt_resize).
RT_HD f2 ld2(const float2* a, size_t i) {
    f2 r;
    r.x = r.y = 0.0f;
    if (a) {
        const float2 v = a[i];
        r.x = v.x;
        r.y = v.y;
    }
    return r;
}

// Extra samples of a pixel from this frame's and the previous frame's motion: extra_samples itself.
RT_HD int extra_count(const Uniforms& U, f2 mv, f2 pm) { return extra_samples(U, max_extra_samples(U), mv, pm); }

// The record of an extra sample a pixel does not take: what rt_shade_hits writes for a ray that
// is not to be traced (zeros, flags 0, tmax = -1).
RT_HD void camera_record_none(CameraWords& w) {
    const float4 z = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    w.r0 = z;
    w.r1 = make_float4(0.0f, 0.0f, 0.0f, -1.0f);
    w.p0 = z;
    w.p1 = z;
    w.p2 = make_uint4(0u, 0u, 0u, 0u);
}

// Samples pixel p of rt_debug_resolve_samples_host holds: spp + extra[p] (extra null: none), at most its stride.
RT_HD uint32_t pixel_samples(const uint32_t* extra, size_t p, uint32_t spp, uint32_t stride) {
    const uint32_t e = extra ? extra[p] : 0u;
    return e < stride - spp ? spp + e : stride;   // spp <= stride (checked by the host)
}

// A pixel of rt_debug_resolve_samples_host: its `count` samples at s summed in sample order, then
// resolve_pixel (the division and, past frame 0, the EMA against history[pix] weighted by the
// motion); alpha 1 as the frame kernels store it.
RT_HD float4 resolve_samples_pixel(const Uniforms& U, const float4* s, uint32_t count, f2 mv, f2 pm, const float4* history,
                                   size_t pix) {
    f3 total = ld3(s[0]);
    for (uint32_t k = 1; k < count; ++k) total = total + ld3(s[k]);
    const f3 c = resolve_pixel(U, total, (int)count, mv, pm, history, pix);
    return make_float4(c.x, c.y, c.z, 1.0f);
}

// ---- compaction: tile geometry ------------------------------------------------------------------------
// A tile is kCompactTile consecutive records, one block's work in the count and the copy launch:
// kCompactSegs segments of 64 records, one selection word (a wave's ballot) each.  The call's
// temporary storage: the selection words of every tile, then one 32-bit count (after the scan:
// offset) per tile.
constexpr uint32_t kCompactTile = 1024;
constexpr uint32_t kCompactSegs = kCompactTile / 64;
constexpr uint32_t kCompactMaxStreams = 4;
RT_HD uint32_t compact_tiles(uint32_t n) { return (n - 1u) / kCompactTile + 1u; }   // n > 0 (a device count of 0: launch_tiles, rt_query.hip)
RT_HD size_t compact_scratch_bytes(uint32_t n) {
    return (size_t)compact_tiles(n) * (kCompactSegs * sizeof(unsigned long long) + sizeof(uint32_t));
}

}  // namespace rt
