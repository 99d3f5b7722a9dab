// rt_scene_host.h — a scene description as host arrays in the layouts the kernels read: what
// rt_scene_upload copies to the device (rt_api_scene.cpp) and what the host debug hooks walk
// (rt_debug_trace_host there, rt_debug_resolve_host in rt_surface_host.cpp), so both see the same
// checks and the same tables.  Internal; header-only.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "rt_ctx.h"

namespace rt {

// What rt_scene_upload accepts; the scene's sizes on success.  c may be null (the debug hooks).
inline rt_status validate_scene(rt_ctx* c, const rt_scene_desc* sd, int& max_sub, uint64_t& nv, uint64_t& nt) {
    if (sd->mesh_count == 0) FAIL(c, RT_ERR_INVALID_ARG, "scene has no meshes");
    if (sd->light_count == 0 || !sd->lights) FAIL(c, RT_ERR_INVALID_ARG, "scene has no lights");
    if (sd->mesh_count >= (1u << 24)) FAIL(c, RT_ERR_UNSUPPORTED, "too many meshes");
    max_sub = 1;
    nv = nt = 0;
    for (uint32_t m = 0; m < sd->mesh_count; ++m) {
        const rt_mesh_desc& md = sd->meshes[m];
        if (!md.positions || !md.normals) FAIL(c, RT_ERR_INVALID_ARG, "mesh without positions/normals");
        if (md.submesh_count == 0 || !md.submeshes) FAIL(c, RT_ERR_INVALID_ARG, "mesh without submeshes");
        if (md.submesh_count > 256) FAIL(c, RT_ERR_UNSUPPORTED, "more than 256 submeshes in a mesh");
        if (md.joint_count && (!md.joint_indices || !md.joint_weights)) FAIL(c, RT_ERR_INVALID_ARG, "skinned mesh without joint streams");
        max_sub = std::max(max_sub, (int)md.submesh_count);
        nv += md.vertex_count;
        for (uint32_t s = 0; s < md.submesh_count; ++s) {
            const rt_submesh_desc& sm = md.submeshes[s];
            if (sm.index_count % 3) FAIL(c, RT_ERR_INVALID_ARG, "index count not a multiple of 3");
            if (sm.index_count && !sm.indices) FAIL(c, RT_ERR_INVALID_ARG, "null indices");
            for (int k = 0; k < RT_TEXTURE_SLOTS; ++k)
                if (k != 4 && (sm.material.textureFlags >> k & 1u) &&   // the AO slot is never sampled
                    (sm.textures[k] < 0 || (uint32_t)sm.textures[k] >= sd->texture_count || !sd->textures))
                    FAIL(c, RT_ERR_INVALID_ARG, "textured material without a valid texture for a flagged slot");
            for (uint32_t i = 0; i < sm.index_count; ++i)
                if (sm.indices[i] >= md.vertex_count) FAIL(c, RT_ERR_INVALID_ARG, "index out of range");
            nt += sm.index_count / 3;
        }
    }
    if (nt >= (1ull << 31) || nv >= (1ull << 32)) FAIL(c, RT_ERR_UNSUPPORTED, "scene too large");
    uint64_t ntexels = 0;
    for (uint32_t t = 0; t < sd->texture_count; ++t) {
        const rt_texture_desc& td = sd->textures[t];
        if (!td.rgba8 || td.width == 0 || td.height == 0) FAIL(c, RT_ERR_INVALID_ARG, "bad texture");
        ntexels += (uint64_t)td.width * td.height;
    }
    if (ntexels >= (1ull << 32)) FAIL(c, RT_ERR_UNSUPPORTED, "texture pool above 2^32 texels");
    return RT_OK;
}

// What rt_shade_hits and rt_debug_shade_host accept of their arguments before they look at the
// lights: opts in range, every pointer but `randoms` set when n > 0, all of them 16-byte aligned.
inline rt_status validate_shade(rt_ctx* c, const rt_shade_opts* o, const void* rays, const void* surfaces,
                                const void* materials, const void* randoms, uint32_t n, const void* paths,
                                const void* next_rays, const void* shadow_rays, const void* contrib) {
    if (!o) FAIL(c, RT_ERR_INVALID_ARG, "null opts");
    if (o->shading_mode != ShadingModePBR && o->shading_mode != ShadingModeLegacy)
        FAIL(c, RT_ERR_INVALID_ARG, "shading_mode is neither ShadingModePBR nor ShadingModeLegacy");
    if (o->max_bounces < 1 || o->max_bounces > RT_MAX_BOUNCES) FAIL(c, RT_ERR_INVALID_ARG, "max_bounces outside 1 .. 12");
    if (o->light_count < 0) FAIL(c, RT_ERR_INVALID_ARG, "negative light_count");
    if (n > 0 && (!rays || !surfaces || !materials || !paths || !next_rays || !shadow_rays || !contrib))
        FAIL(c, RT_ERR_INVALID_ARG, "null argument");
    if (((uintptr_t)rays | (uintptr_t)surfaces | (uintptr_t)materials | (uintptr_t)randoms | (uintptr_t)paths |
         (uintptr_t)next_rays | (uintptr_t)shadow_rays | (uintptr_t)contrib) & 15u)
        FAIL(c, RT_ERR_INVALID_ARG, "every record array must be 16-byte aligned");
    return RT_OK;
}
// opts->light_count against the lights there are: 0 = all of them.
inline rt_status shade_light_count(rt_ctx* c, const rt_shade_opts* o, uint32_t have, int& count) {
    count = o->light_count ? o->light_count : (int)have;
    if (count < 1) FAIL(c, RT_ERR_INVALID_ARG, "no lights");
    if ((uint32_t)count > have) FAIL(c, RT_ERR_INVALID_ARG, "light_count above the lights there are");
    return RT_OK;
}

// What rt_camera_paths and rt_debug_camera_paths_host accept of their arguments (the offsets'
// source apart: the context's own or the caller's).
inline rt_status validate_camera(rt_ctx* c, const Uniforms* u, const rt_camera_opts* o, const void* random_offsets,
                                 uint32_t n, const void* rays, const void* paths) {
    if (!u || !o) FAIL(c, RT_ERR_INVALID_ARG, "null uniforms / opts");
    if (u->width <= 0 || u->height <= 0 || (int64_t)u->width * u->height > (1ll << 30))
        FAIL(c, RT_ERR_INVALID_ARG, "bad size");
    if (o->sample < 0) FAIL(c, RT_ERR_INVALID_ARG, "negative sample");
    if (o->tag_stride == 0) FAIL(c, RT_ERR_INVALID_ARG, "tag_stride is 0");
    if ((uint64_t)o->first_pixel + n > (uint64_t)u->width * (uint64_t)u->height)
        FAIL(c, RT_ERR_INVALID_ARG, "first_pixel + n is past the image");
    if (n > 0 && (!rays || !paths)) FAIL(c, RT_ERR_INVALID_ARG, "null argument");
    if ((((uintptr_t)rays | (uintptr_t)paths) & 15u) || ((uintptr_t)random_offsets & 3u))
        FAIL(c, RT_ERR_INVALID_ARG, "rays and paths must be 16-byte aligned, random_offsets 4-byte aligned");
    return RT_OK;
}

// What rt_compact_paths and rt_debug_compact_paths_host accept.  Overlap cannot be checked in
// full: equal base pointers are.
inline rt_status validate_compact(rt_ctx* c, const void* paths, uint32_t n, uint32_t mask, const rt_compact_stream* streams,
                                  uint32_t stream_count, const void* index, const void* count) {
    if (mask == 0) FAIL(c, RT_ERR_INVALID_ARG, "mask is 0");
    if (stream_count > 4) FAIL(c, RT_ERR_INVALID_ARG, "more than 4 streams");
    if (stream_count > 0 && !streams) FAIL(c, RT_ERR_INVALID_ARG, "null streams");
    for (uint32_t k = 0; k < stream_count; ++k)
        if (streams[k].words < 1 || streams[k].words > 4) FAIL(c, RT_ERR_INVALID_ARG, "stream words outside 1 .. 4");
    if (n == 0) return RT_OK;
    if (!paths || !count) FAIL(c, RT_ERR_INVALID_ARG, "null argument");
    if (((uintptr_t)paths & 15u) || (((uintptr_t)index | (uintptr_t)count) & 3u))
        FAIL(c, RT_ERR_INVALID_ARG, "paths must be 16-byte aligned, index and count 4-byte aligned");
    if (count == paths || count == index || (index && index == paths))
        FAIL(c, RT_ERR_INVALID_ARG, "index, count and paths overlap");
    for (uint32_t k = 0; k < stream_count; ++k) {
        const rt_compact_stream& s = streams[k];
        if (!s.src || !s.dst) FAIL(c, RT_ERR_INVALID_ARG, "null stream pointer");
        if (((uintptr_t)s.src | (uintptr_t)s.dst) & 15u) FAIL(c, RT_ERR_INVALID_ARG, "stream pointers must be 16-byte aligned");
        if (s.dst == paths || s.dst == index || s.dst == count || s.src == count || (index && s.src == index))
            FAIL(c, RT_ERR_INVALID_ARG, "a stream overlaps paths, index or count (in place is not supported)");
        for (uint32_t j = 0; j < stream_count; ++j)
            if (s.dst == streams[j].src || (j != k && s.dst == streams[j].dst))
                FAIL(c, RT_ERR_INVALID_ARG, "a dst equals a src or another dst (in place is not supported)");
    }
    return RT_OK;
}

// What the temporal host hooks accept (the scene apart).
inline rt_status validate_primary(rt_ctx* c, const Uniforms* u, const rt_target_opts* o, const void* hits, const void* paths,
                                  uint32_t n, const void* depth, const void* motion) {
    if (!u || !o) FAIL(c, RT_ERR_INVALID_ARG, "null uniforms / opts");
    if (o->tag_stride == 0) FAIL(c, RT_ERR_INVALID_ARG, "tag_stride is 0");
    if (o->tag_offset >= o->tag_stride) FAIL(c, RT_ERR_INVALID_ARG, "tag_offset is not below tag_stride");
    if (n > 0 && (!hits || !paths || !depth || !motion)) FAIL(c, RT_ERR_INVALID_ARG, "null argument");
    if ((((uintptr_t)hits | (uintptr_t)paths) & 15u) || ((uintptr_t)motion & 7u) || ((uintptr_t)depth & 3u))
        FAIL(c, RT_ERR_INVALID_ARG, "hits and paths must be 16-byte aligned, motion 8-byte, depth 4-byte");
    return RT_OK;
}
// rt_camera_paths' checks, but that rays / paths may be null when no pixel can take an extra sample
// (max_extra: max_extra_samples of u, 0 for a null u).
inline rt_status validate_extra(rt_ctx* c, const Uniforms* u, const rt_camera_opts* o, const void* random_offsets,
                                const void* motion, const void* motion_prev, uint32_t n, const void* rays, const void* paths,
                                const void* extra, int max_extra) {
    if (rt_status st = validate_camera(c, u, o, random_offsets, 0, rays, paths)) return st;
    if ((uint64_t)o->first_pixel + n > (uint64_t)u->width * (uint64_t)u->height)
        FAIL(c, RT_ERR_INVALID_ARG, "first_pixel + n is past the image");
    if (n > 0 && (!motion || !extra)) FAIL(c, RT_ERR_INVALID_ARG, "null motion / extra");
    if (n > 0 && max_extra > 0 && (!rays || !paths)) FAIL(c, RT_ERR_INVALID_ARG, "null rays / paths with extra samples enabled");
    if ((((uintptr_t)motion | (uintptr_t)motion_prev) & 7u) || ((uintptr_t)extra & 3u))
        FAIL(c, RT_ERR_INVALID_ARG, "motion targets must be 8-byte aligned, extra 4-byte aligned");
    if (u->samplesPerPixel > 4096 || max_extra > 4096) FAIL(c, RT_ERR_INVALID_ARG, "bad spp");   // as rt_render_frame
    if (o->sample > 0x7fffffff - max_extra) FAIL(c, RT_ERR_INVALID_ARG, "sample + the most extra samples overflows");
    return RT_OK;
}
inline rt_status validate_resolve_samples(rt_ctx* c, const Uniforms* u, const void* samples, uint32_t stride,
                                          const void* extra, const void* motion, const void* motion_prev, const void* history,
                                          uint32_t pixels, const void* rgba, int max_extra) {
    if (!u) FAIL(c, RT_ERR_INVALID_ARG, "null uniforms");
    if (u->samplesPerPixel < 1 || u->samplesPerPixel > 64) FAIL(c, RT_ERR_INVALID_ARG, "samplesPerPixel outside 1 .. 64");
    if ((uint64_t)u->samplesPerPixel + (uint64_t)max_extra > (uint64_t)stride)
        FAIL(c, RT_ERR_INVALID_ARG, "samplesPerPixel + the most extra samples is more than sample_stride");
    if (u->frameIndex > 0 && !history) FAIL(c, RT_ERR_INVALID_ARG, "null history past frame 0");
    if (pixels > 0) {
        if (!samples || !rgba) FAIL(c, RT_ERR_INVALID_ARG, "null argument");
        if (rgba == history || rgba == samples) FAIL(c, RT_ERR_INVALID_ARG, "in place is not supported");
    }
    if ((((uintptr_t)samples | (uintptr_t)history | (uintptr_t)rgba) & 15u) ||
        (((uintptr_t)motion | (uintptr_t)motion_prev) & 7u) || ((uintptr_t)extra & 3u))
        FAIL(c, RT_ERR_INVALID_ARG, "samples, history and rgba must be 16-byte aligned, motion targets 8-byte, extra 4-byte");
    return RT_OK;
}

// A scene description flattened mesh by mesh: positions and normals with every mesh's vertices
// after the previous one's, triangles as (three vertex ids, mesh << 8 | submesh), 12 floats of
// transform per mesh.  nrm may be null.
inline void flatten_scene(const rt_scene_desc* sd, std::vector<float4>& pos, std::vector<float4>* nrm,
                          std::vector<uint4>& tri_info, std::vector<float>& inst) {
    pos.clear();
    tri_info.clear();
    if (nrm) nrm->clear();
    inst.assign(12 * (size_t)sd->mesh_count, 0.0f);
    for (uint32_t m = 0; m < sd->mesh_count; ++m) {
        const rt_mesh_desc& md = sd->meshes[m];
        const uint32_t vbase = (uint32_t)pos.size();
        std::memcpy(&inst[12 * (size_t)m], &md.transform, 48);
        for (uint32_t v = 0; v < md.vertex_count; ++v) {
            const rt_float3& p = md.positions[v];
            pos.push_back(make_float4(p.x, p.y, p.z, 0.0f));
            if (nrm) nrm->push_back(make_float4(md.normals[v].x, md.normals[v].y, md.normals[v].z, 0.0f));
        }
        for (uint32_t s = 0; s < md.submesh_count; ++s) {
            const rt_submesh_desc& sm = md.submeshes[s];
            for (uint32_t k = 0; k < sm.index_count / 3; ++k)
                tri_info.push_back(make_uint4(vbase + sm.indices[3 * k + 0], vbase + sm.indices[3 * k + 1],
                                              vbase + sm.indices[3 * k + 2], (m << 8) | s));
        }
    }
}

// Texture path: the texel pool, its table, every material slot's texture
// ids and the per-vertex UVs (Model.vertexDescriptor's zero default when a mesh has none,
// Model.swift:329-333).  Only mat_tex and `textured` are filled in for an untextured scene.
struct TexTables {
    bool textured = false;
    std::vector<int4> mat_tex;      // DevScene::mat_tex
    std::vector<uint4> info;        // DevScene::tex_info
    std::vector<uint8_t> texels;    // DevScene::tex_texels
    std::vector<float2> uv;         // DevScene::uv
    float lut[512];                 // DevScene::tex_lut
};
inline void build_tex_tables(const rt_scene_desc* sd, int max_sub, uint32_t num_verts, TexTables& T) {
    const uint32_t slots = (uint32_t)max_sub * sd->mesh_count;
    T.mat_tex.assign(2 * (size_t)slots, make_int4(0, -1, -1, -1));
    T.textured = false;
    for (uint32_t m = 0; m < sd->mesh_count; ++m)
        for (uint32_t s = 0; s < sd->meshes[m].submesh_count; ++s) {
            const rt_submesh_desc& sm = sd->meshes[m].submeshes[s];
            uint32_t flags = sm.material.textureFlags & ~(1u << 4);   // ENABLE_AO = 0
            if (!flags) continue;
            T.textured = true;
            int t[8];
            for (int k = 0; k < 8; ++k) t[k] = (k < RT_TEXTURE_SLOTS && (flags >> k & 1u)) ? sm.textures[k] : -1;
            const size_t slot = (size_t)m * max_sub + s;
            T.mat_tex[2 * slot] = make_int4((int)flags, t[0], t[1], t[2]);
            T.mat_tex[2 * slot + 1] = make_int4(t[3], t[4], t[5], t[6]);
        }
    if (!T.textured) return;
    T.info.resize(sd->texture_count);
    uint64_t off = 0;
    for (uint32_t t = 0; t < sd->texture_count; ++t) {
        const rt_texture_desc& td = sd->textures[t];
        T.info[t] = make_uint4((uint32_t)off, td.width, td.height, 0u);
        off += (uint64_t)td.width * td.height;
    }
    T.texels.resize(off * 4);
    for (uint32_t t = 0; t < sd->texture_count; ++t)
        std::memcpy(&T.texels[4 * (size_t)T.info[t].x], sd->textures[t].rgba8, 4 * (size_t)T.info[t].y * T.info[t].z);
    T.uv.assign(num_verts, make_float2(0.0f, 0.0f));
    uint32_t vbase = 0;
    for (uint32_t m = 0; m < sd->mesh_count; ++m) {
        const rt_mesh_desc& md = sd->meshes[m];
        if (md.uvs)
            for (uint32_t v = 0; v < md.vertex_count; ++v) T.uv[vbase + v] = make_float2(md.uvs[v].x, md.uvs[v].y);
        vbase += md.vertex_count;
    }
    // texel byte -> float: [0, 256) linear b / 255, [256, 512) sRGB EOTF (MTKTextureLoader .SRGB)
    for (int b = 0; b < 256; ++b) {
        const double v = b / 255.0;
        T.lut[b] = (float)v;
        T.lut[256 + b] = (float)(v <= 0.04045 ? v / 12.92 : std::pow((v + 0.055) / 1.055, 2.4));
    }
}

}  // namespace rt
