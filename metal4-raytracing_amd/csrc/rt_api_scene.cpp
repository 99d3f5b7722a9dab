// rt_api_scene.cpp — what frames read: scene upload and textures, the BVH (host build, device
// build, refit and its quality check), skinning and instance transforms, all into the geometry
// generation the frame ring names (rt_frame_ring.h).  Also the host debug tracer, which builds
// the same tree from a scene description.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <exception>

#include "rt_ctx.h"
#include "rt_scene_host.h"

using namespace rt;

namespace {
// SAH build (one triangle per BVH2 leaf) + SAH-DP 8-wide collapse (c_node 1, c_prim 0.5: the C3g
// sweep of DESIGN.md §3) whose group-stack depth fits the kStackSize LDS stack: the binned-SAH
// builder falls back to median splits past its depth limit, so tighter limits bound the depth.
// false on failure (no depth limit fits, or the builder threw: allocation, internal checks);
// nothing is thrown across the C-ABI.
bool build_bvh8_fit(const float* world, uint32_t n, BvhResult& b2, Bvh8Result& b8) {
    try {
        for (int limit : {64, 48, 40, 32, 28, 24, 21}) {
            b2 = build_bvh2(world, n, 1, limit);
            b8 = collapse_bvh8_dp(b2, 1.0f, 0.5f);
            if (b8.max_depth <= kStackSize) return true;
        }
    } catch (const std::exception&) {
    }
    return false;
}

// host object->world, identical arithmetic to rt::xform on the device
void xform_host(const float* m, const float4& p, float* out) {
    for (int r = 0; r < 3; ++r) out[r] = ((m[0 + r] * p.x + m[3 + r] * p.y) + m[6 + r] * p.z) + m[9 + r] * 1.0f;
}

// World-space triangles (9 floats each) in the original order, from object-space positions and
// each triangle's instance transform (tri_info.w >> 8 = mesh).
void world_tris(const std::vector<uint4>& tri_info, const std::vector<float4>& pos, const std::vector<float>& inst,
                std::vector<float>& world) {
    world.resize(9 * tri_info.size());
    for (size_t t = 0; t < tri_info.size(); ++t) {
        const uint4& ti = tri_info[t];
        const float* M = &inst[12 * (ti.w >> 8)];
        xform_host(M, pos[ti.x], &world[9 * t + 0]);
        xform_host(M, pos[ti.y], &world[9 * t + 3]);
        xform_host(M, pos[ti.z], &world[9 * t + 6]);
    }
}

// The traversal's 64-B triangle records (rt_device.h) in the tree's slot order.
std::vector<float> slot_ordered_tris(const std::vector<float>& world, const std::vector<uint32_t>& tri_order) {
    std::vector<float> tris((size_t)kTriFloats * tri_order.size());
    for (size_t k = 0; k < tri_order.size(); ++k) {
        const uint32_t id = tri_order[k];
        tri_store(&tris[(size_t)kTriFloats * k], &world[9 * (size_t)id], id);
    }
    return tris;
}

// Before a geometry update: the first one after a frame switches to the next generation, once the
// frames still reading it have finished, seeded with a copy of the current one (on the update
// stream; frames keep reading the current generation meanwhile).  Every entry point that writes
// geometry or the tree (skinning, transforms, refit, both builds and with them the automatic
// rebuild) comes through here first, so this is also where they wait for pending ray queries: a
// query reads the newest generation, which an update without a frame in between rewrites in place.
rt_status begin_update(rt_ctx* c) {
    if (rt_status st = drain_queries(c)) return st;
    const UpdatePlan u = c->ring.plan_update();
    if (!u.seed) return RT_OK;
    for (int k = 0; k < kMaxSlots; ++k)
        if (u.wait[k]) HIPC(c, hipEventSynchronize(c->slot[k].done));
    Geo& src = c->geo[u.src];
    Geo& dst = c->geo[u.dst];
    for (int i = 0; i < Geo::kCount; ++i) {
        if (rt_status st = dev_alloc(c, dst.buf[i], src.buf[i].bytes)) return st;
        if (src.buf[i].bytes)
            HIPC(c, hipMemcpyAsync(dst.buf[i].p, src.buf[i].p, src.buf[i].bytes, hipMemcpyDeviceToDevice, c->ustream));
    }
    dst.num_nodes8 = src.num_nodes8;
    c->ring.commit_update();
    return RT_OK;
}

// The texture tables of a textured scene (build_tex_tables, rt_scene_host.h).  Nothing is
// uploaded for an untextured scene.
rt_status upload_textures(rt_ctx* c, const rt_scene_desc* sd) {
    TexTables T;
    build_tex_tables(sd, c->max_sub, c->num_verts, T);
    c->textured = T.textured;
    if (!T.textured) return RT_OK;
    rt_status st;
    if ((st = dev_upload(c, c->d_tex_texels, T.texels.data(), T.texels.size()))) return st;
    if ((st = dev_upload(c, c->d_tex_info, T.info.data(), T.info.size() * sizeof(uint4)))) return st;
    if ((st = dev_upload(c, c->d_mat_tex, T.mat_tex.data(), T.mat_tex.size() * sizeof(int4)))) return st;
    if ((st = dev_upload(c, c->d_uv, T.uv.data(), T.uv.size() * sizeof(float2)))) return st;
    if ((st = dev_upload(c, c->d_tex_lut, T.lut, sizeof T.lut))) return st;
    return RT_OK;
}

// rest pose + joint streams of every skinned mesh (positions of static meshes unused)
rt_status upload_skinning(rt_ctx* c, const rt_scene_desc* sd) {
    const size_t nv = c->num_verts;
    std::vector<uint16_t> jidx(4 * nv, 0);
    std::vector<float> jw(4 * nv, 0.0f);
    uint32_t maxj = 0;
    for (uint32_t m = 0; m < sd->mesh_count; ++m) {
        const rt_mesh_desc& md = sd->meshes[m];
        if (!md.joint_count) continue;
        maxj = std::max(maxj, md.joint_count);
        std::memcpy(&jidx[4 * (size_t)c->meshes[m].vbase], md.joint_indices, 8 * (size_t)md.vertex_count);
        std::memcpy(&jw[4 * (size_t)c->meshes[m].vbase], md.joint_weights, 16 * (size_t)md.vertex_count);
    }
    rt_status st;
    if ((st = dev_upload(c, c->d_rest_pos, c->h_pos.data(), nv * 16))) return st;
    if ((st = dev_upload(c, c->d_rest_nrm, c->h_nrm.data(), nv * 16))) return st;
    if ((st = dev_upload(c, c->d_jidx, jidx.data(), jidx.size() * 2))) return st;
    if ((st = dev_upload(c, c->d_jw, jw.data(), jw.size() * 4))) return st;
    return dev_alloc(c, c->d_joints, (size_t)maxj * 64);
}

// The node-area sum of the current generation's tree (launch_bvh_cost) on the update stream: read
// back at once (sync = true, after a build) or into the pinned word with an event (after a refit).
// The exact boxes of the root's children (launch_root_boxes) of the current generation's tree, on the
// update stream: after the tree's upload, the device build and every refit.
rt_status root_boxes(rt_ctx* c) {
    Geo& g = c->G();
    if (rt_status st = dev_alloc(c, g[Geo::root_box], sizeof(RootBoxes))) return st;
    launch_root_boxes((const Bvh8Node*)g[Geo::nodes].p, (const float*)g[Geo::node_box].p, (const float*)g[Geo::tris].p,
                      (RootBoxes*)g[Geo::root_box].p, c->ustream);
    HIPC(c, hipGetLastError());
    return RT_OK;
}

rt_status bvh_cost(rt_ctx* c, bool sync) {
    if (rt_status st = dev_alloc(c, c->d_cost, 4)) return st;
    if (!c->h_cost) HIPC(c, c->h_cost.alloc(16));
    if (!c->cost_ev) HIPC(c, c->cost_ev.create(hipEventDisableTiming));
    launch_bvh_cost((const float*)c->G()[Geo::node_box].p, c->num_nodes8, (float*)c->d_cost.p, c->ustream);
    HIPC(c, hipGetLastError());
    HIPC(c, hipMemcpyAsync(c->h_cost, c->d_cost.p, 4, hipMemcpyDeviceToHost, c->ustream));
    if (sync) {
        HIPC(c, hipStreamSynchronize(c->ustream));
        c->stats.bvh_cost_built = *c->h_cost.get();   // bvh_cost_refit keeps the last refit's figure
        c->cost_pending = false;
    } else {
        HIPC(c, hipEventRecord(c->cost_ev, c->ustream));
        c->cost_pending = true;
    }
    return RT_OK;
}
}  // namespace

// Once the last refit's node-area sum has arrived: if it grew past refit_rebuild_pct percent of
// the last build's, rebuild on the device from the current geometry (the reference rebuilds its
// acceleration structures where a refit is not enough, Renderer.swift:1252-1277).  Images do not
// depend on the tree (conservative boxes): this only restores traversal speed.
rt_status check_refit_quality(rt_ctx* c, bool* rebuilt) {
    *rebuilt = false;
    if (!c->cost_pending || hipEventQuery(c->cost_ev) != hipSuccess) return RT_OK;
    c->cost_pending = false;
    const float built = c->stats.bvh_cost_built, refit = c->stats.bvh_cost_refit = *c->h_cost.get();
    const int pct = refit_rebuild_pct(c);
    if (pct <= 0 || !(built > 0.0f) || !(refit * 100.0f > built * (float)pct)) return RT_OK;
    if (rt_status st = rt_bvh_build_device(c)) return st;
    c->stats.total_auto_rebuilds++;
    *rebuilt = true;
    return RT_OK;
}

extern "C" {

rt_status rt_scene_upload(rt_ctx* c, const rt_scene_desc* sd) {
    if (!c || !sd) FAIL(c, RT_ERR_INVALID_ARG, "null argument");
    if (rt_status dst = drain_frames(c)) return dst;
    if (rt_status qst = drain_queries(c)) return qst;
    HIPC(c, hipSetDevice(c->device));
    int max_sub;
    uint64_t nv, nt;
    rt_status st;
    if ((st = validate_scene(c, sd, max_sub, nv, nt))) return st;
    c->max_sub = max_sub;
    c->num_inst = sd->mesh_count;
    c->num_tris = (uint32_t)nt;
    c->num_verts = (uint32_t)nv;
    flatten_scene(sd, c->h_pos, &c->h_nrm, c->h_tri_info, c->h_inst);
    world_tris(c->h_tri_info, c->h_pos, c->h_inst, c->h_world);
    Material zero_mat;
    std::memset(&zero_mat, 0, sizeof zero_mat);
    c->h_mat.assign((size_t)max_sub * sd->mesh_count, zero_mat);
    c->meshes.assign(sd->mesh_count, MeshInfo());
    uint32_t vbase = 0, tri = 0;
    bool any_skin = false;
    // ray queries' primitive ids: the first scene-wide triangle id of every submesh
    std::vector<uint32_t> sub_first((size_t)max_sub * sd->mesh_count, 0u);
    for (uint32_t m = 0; m < sd->mesh_count; ++m) {
        const rt_mesh_desc& md = sd->meshes[m];
        MeshInfo& mi = c->meshes[m];
        mi.vbase = vbase;
        mi.vcount = md.vertex_count;
        mi.tbase = tri;
        mi.joint_count = md.joint_count;
        mi.skinned = md.joint_count > 0;
        any_skin |= mi.skinned;
        for (uint32_t s = 0; s < md.submesh_count; ++s) {
            c->h_mat[(size_t)m * max_sub + s] = md.submeshes[s].material;
            sub_first[(size_t)m * max_sub + s] = tri;
            tri += md.submeshes[s].index_count / 3;
        }
        vbase += md.vertex_count;
        mi.tcount = tri - mi.tbase;
    }
    c->h_lights.assign(sd->lights, sd->lights + sd->light_count);
    Geo& g = c->G();
    if ((st = upload_textures(c, sd))) return st;
    if ((st = dev_upload(c, g[Geo::pos], c->h_pos.data(), nv * 16))) return st;
    if ((st = dev_upload(c, g[Geo::prev_pos], c->h_pos.data(), nv * 16))) return st;  // previousPositions = positions (SubMesh.swift:60)
    if ((st = dev_upload(c, g[Geo::nrm], c->h_nrm.data(), nv * 16))) return st;
    if ((st = dev_upload(c, c->d_tri_info, c->h_tri_info.data(), nt * 16))) return st;
    if ((st = dev_alloc(c, g[Geo::tri_nrm], nt * 64))) return st;
    launch_tri_nrm((const uint4*)c->d_tri_info.p, (const float4*)g[Geo::nrm].p, (float4*)g[Geo::tri_nrm].p, 0,
                   (uint32_t)nt, c->stream);
    c->ring.ctx_work++;
    HIPC(c, hipGetLastError());
    if ((st = dev_upload(c, g[Geo::inst], c->h_inst.data(), c->h_inst.size() * 4))) return st;
    if ((st = dev_upload(c, g[Geo::prev_inst], c->h_inst.data(), c->h_inst.size() * 4))) return st;
    if ((st = dev_upload(c, c->d_mat, c->h_mat.data(), c->h_mat.size() * sizeof(Material)))) return st;
    if ((st = dev_upload(c, c->d_lights, c->h_lights.data(), c->h_lights.size() * sizeof(Light)))) return st;
    if ((st = dev_upload(c, c->d_sub_first, sub_first.data(), sub_first.size() * 4))) return st;
    if (any_skin && (st = upload_skinning(c, sd))) return st;
    HIPC(c, hipStreamSynchronize(c->stream));
    c->scene_ready = true;
    c->bvh_ready = false;
    c->inst_moved = c->skin_moved = c->last_moving = false;
    return RT_OK;
}

rt_status rt_bvh_build(rt_ctx* c) {
    if (!c) FAIL(c, RT_ERR_INVALID_ARG, "null ctx");
    if (!c->scene_ready) FAIL(c, RT_ERR_STATE, "rt_bvh_build before rt_scene_upload");
    HIPC(c, hipSetDevice(c->device));
    // into the update generation: frames in flight keep theirs (and their tree)
    if (rt_status ust = begin_update(c)) return ust;
    HIPC(c, hipStreamSynchronize(c->ustream));
    Geo& g = c->G();
    // current world-space triangles (may have been skinned / re-transformed on the device)
    if (c->world_dirty) {
        HIPC(c, hipMemcpy(c->h_pos.data(), g[Geo::pos].p, (size_t)c->num_verts * 16, hipMemcpyDeviceToHost));
        world_tris(c->h_tri_info, c->h_pos, c->h_inst, c->h_world);
        c->world_dirty = false;
    }
    // the size the host and device builders are tested to (the device build's 64-bit Morton keys
    // carry the triangle id beside the Morton bits)
    if (c->num_tris >= (1u << 26)) FAIL(c, RT_ERR_UNSUPPORTED, "more than 2^26 triangles");
    if (!build_bvh8_fit(c->h_world.data(), c->num_tris, c->bvh, c->bvh8))
        FAIL(c, RT_ERR_UNSUPPORTED, "BVH deeper than the traversal stack at every depth limit");
    if (c->bvh8.nodes.size() >= (1u << 23)) FAIL(c, RT_ERR_UNSUPPORTED, "BVH too large (2^23 nodes)");
    const uint32_t n = c->num_tris;
    const std::vector<float> tris = slot_ordered_tris(c->h_world, c->bvh8.tri_order);
    // nodes grouped by depth for the level-synchronous refit (BFS order: parent < child)
    const size_t nn = c->bvh8.nodes.size();
    std::vector<int> depth(nn, 0);
    int maxd = 0;
    for (size_t k = 1; k < nn; ++k) {
        depth[k] = depth[c->bvh8.parent[k]] + 1;
        maxd = std::max(maxd, depth[k]);
    }
    c->level_off.assign(maxd + 2, 0);
    for (int d : depth) c->level_off[d + 1]++;
    for (int d = 0; d <= maxd; ++d) c->level_off[d + 1] += c->level_off[d];
    c->level_nodes.assign(nn, 0);
    std::vector<uint32_t> fill(c->level_off.begin(), c->level_off.end() - 1);
    for (size_t k = 0; k < nn; ++k) c->level_nodes[fill[depth[k]]++] = (uint32_t)k;
    rt_status st;
    hipStream_t us = c->ustream;
    if ((st = dev_upload(c, g[Geo::tris], tris.data(), tris.size() * 4, us))) return st;
    if ((st = dev_upload(c, g[Geo::nodes], c->bvh8.nodes.data(), nn * sizeof(Bvh8Node), us))) return st;
    if ((st = dev_upload(c, g[Geo::node_box], c->bvh8.node_box.data(), c->bvh8.node_box.size() * 4, us))) return st;
    if ((st = dev_upload(c, c->d_slot_to_tri, c->bvh8.tri_order.data(), (size_t)n * 4, us))) return st;
    if ((st = dev_upload(c, c->d_levels, c->level_nodes.data(), c->level_nodes.size() * 4, us))) return st;
    // hit-sort keys: the leaf-order bin of every triangle (DevScene::tri_bin)
    std::vector<uint16_t> tri_bin(n);
    for (uint32_t k = 0; k < n; ++k) tri_bin[c->bvh8.tri_order[k]] = (uint16_t)(((uint64_t)k * kSortMaxBins) / n);
    if ((st = dev_upload(c, g[Geo::tri_bin], tri_bin.data(), (size_t)n * 2, us))) return st;
    c->num_nodes8 = (uint32_t)nn;
    if ((st = root_boxes(c))) return st;
    if ((st = bvh_cost(c, true))) return st;
    HIPC(c, hipStreamSynchronize(us));   // the host arrays are the copies' sources
    g.num_nodes8 = (uint32_t)nn;
    c->num_nodes8 = (uint32_t)nn;
    c->bvh_ready = true;
    return RT_OK;
}

rt_status rt_bvh_build_device(rt_ctx* c) {
    if (!c) FAIL(c, RT_ERR_INVALID_ARG, "null ctx");
    if (!c->scene_ready) FAIL(c, RT_ERR_STATE, "rt_bvh_build_device before rt_scene_upload");
    if (c->num_tris < 2) return rt_bvh_build(c);   // nothing to sort: the host path is exact and instant
    if (c->num_tris >= (1u << 26)) FAIL(c, RT_ERR_UNSUPPORTED, "more than 2^26 triangles");
    HIPC(c, hipSetDevice(c->device));
    // into the update generation on the update stream: frames in flight keep their tree
    rt_status st = begin_update(c);
    if (st) return st;
    const uint32_t n = c->num_tris;
    hipStream_t us = c->ustream;
    if ((st = dev_alloc(c, c->d_lbvh_scratch, lbvh_scratch_bytes(n)))) return st;
    Geo& g = c->G();
    if ((st = dev_alloc(c, g[Geo::nodes], (size_t)n * sizeof(Bvh8Node)))) return st;
    if ((st = dev_alloc(c, g[Geo::node_box], (size_t)n * 6 * sizeof(float)))) return st;
    if ((st = dev_alloc(c, c->d_slot_to_tri, (size_t)n * 4))) return st;
    if ((st = dev_alloc(c, g[Geo::tri_bin], (size_t)n * 2))) return st;
    if ((st = dev_alloc(c, c->d_levels, (size_t)n * 4))) return st;
    if ((st = dev_alloc(c, g[Geo::tris], (size_t)n * kTriFloats * 4))) return st;
    if ((st = dev_alloc(c, c->d_maxabs, 4))) return st;
    if (!c->h_lbvh) HIPC(c, c->h_lbvh.alloc(16));
    LbvhInput in{(const float4*)g[Geo::pos].p, (const uint4*)c->d_tri_info.p, (const float*)g[Geo::inst].p, n};
    // PLOC topology + SAH-DP collapse by default; RT_DEVICE_BVH=lbvh selects the radix tree, whose
    // faster build wins for a small scene rebuilt every frame
    in.ploc = c->tuning_req.device_bvh == 1 ? 0 : 1;   // rt_tuning.device_bvh: 1 = the LBVH radix tree
    LbvhOutput out{(Bvh8Node*)g[Geo::nodes].p, (float*)g[Geo::node_box].p, (uint32_t*)c->d_slot_to_tri.p,
                   (uint16_t*)g[Geo::tri_bin].p, (uint32_t*)c->d_levels.p, c->h_lbvh.get()};
    LbvhResult res;
    const char* err = nullptr;
    if (!lbvh_build(in, out, c->d_lbvh_scratch.p, us, &res, &err)) {
        c->bvh_ready = false;
        FAIL(c, RT_ERR_UNSUPPORTED, std::string("device BVH build: ") + (err ? err : "?"));
    }
    // world-space triangles in the new slot order
    HIPC(c, hipMemsetAsync(c->d_maxabs.p, 0, 4, us));
    launch_flatten((const uint4*)c->d_tri_info.p, (const uint32_t*)c->d_slot_to_tri.p, (const float4*)g[Geo::pos].p,
                   (const float*)g[Geo::inst].p, (float*)g[Geo::tris].p, n, (unsigned*)c->d_maxabs.p, us);
    HIPC(c, hipGetLastError());
    if ((st = root_boxes(c))) return st;
    HIPC(c, hipStreamSynchronize(us));
    if (res.num_nodes >= (1u << 23)) FAIL(c, RT_ERR_UNSUPPORTED, "BVH too large (2^23 nodes)");
    c->level_off = res.level_off;
    c->bvh8 = Bvh8Result();            // the host copy describes the host builder's trees only
    c->bvh8.pad = res.pad;
    c->bvh8.max_depth = res.max_depth;
    c->num_nodes8 = res.num_nodes;
    g.num_nodes8 = res.num_nodes;
    c->bvh_ready = true;
    return bvh_cost(c, true);
}

rt_status rt_bvh_refit(rt_ctx* c) {
    if (!c) FAIL(c, RT_ERR_INVALID_ARG, "null ctx");
    if (!c->bvh_ready) FAIL(c, RT_ERR_STATE, "rt_bvh_refit before rt_bvh_build");
    HIPC(c, hipSetDevice(c->device));
    bool rebuilt = false;
    if (rt_status qst = check_refit_quality(c, &rebuilt)) return qst;
    if (rebuilt) return RT_OK;         // the new tree is built from the current geometry
    rt_status st = begin_update(c);   // frames in flight keep their generation
    if (!st) st = dev_alloc(c, c->d_maxabs, 4);
    if (st) return st;
    Geo& g = c->G();
    HIPC(c, hipMemsetAsync(c->d_maxabs.p, 0, 4, c->ustream));
    launch_flatten((const uint4*)c->d_tri_info.p, (const uint32_t*)c->d_slot_to_tri.p, (const float4*)g[Geo::pos].p,
                   (const float*)g[Geo::inst].p, (float*)g[Geo::tris].p, c->num_tris, (unsigned*)c->d_maxabs.p,
                   c->ustream);
    for (int d = (int)c->level_off.size() - 2; d >= 0; --d) {
        uint32_t off = c->level_off[d], cnt = c->level_off[d + 1] - off;
        launch_refit8_level((Bvh8Node*)g[Geo::nodes].p, (float*)g[Geo::node_box].p, (const float*)g[Geo::tris].p,
                            (const uint32_t*)c->d_levels.p + off, cnt, c->bvh8.pad, (const unsigned*)c->d_maxabs.p,
                            c->ustream);
    }
    HIPC(c, hipGetLastError());
    if ((st = root_boxes(c))) return st;
    // the refitted tree's node-area sum, read back without a host wait (check_refit_quality)
    if (refit_rebuild_pct(c) > 0) return bvh_cost(c, false);
    return RT_OK;
}

rt_status rt_set_instance_transforms(rt_ctx* c, const rt_packed_float4x3* t, uint32_t count) {
    if (!c || !t) FAIL(c, RT_ERR_INVALID_ARG, "null argument");
    if (!c->scene_ready || count != c->num_inst) FAIL(c, RT_ERR_INVALID_ARG, "transform count != mesh count");
    HIPC(c, hipSetDevice(c->device));
    if (rt_status st = begin_update(c)) return st;   // frames in flight keep their generation
    Geo& g = c->G();
    // prev <- cur (Renderer.swift:939-944), then the new transforms
    HIPC(c, hipMemcpyAsync(g[Geo::prev_inst].p, g[Geo::inst].p, c->h_inst.size() * 4, hipMemcpyDeviceToDevice, c->ustream));
    c->inst_moved = std::memcmp(c->h_inst.data(), t, (size_t)count * 48) != 0;
    std::memcpy(c->h_inst.data(), t, (size_t)count * 48);
    HIPC(c, hipMemcpyAsync(g[Geo::inst].p, c->h_inst.data(), c->h_inst.size() * 4, hipMemcpyHostToDevice, c->ustream));
    HIPC(c, hipStreamSynchronize(c->ustream));   // h_inst is the copy's source
    c->world_dirty = true;
    return RT_OK;
}

rt_status rt_skin(rt_ctx* c, uint32_t mesh_index, const float* joints, uint32_t joint_count) {
    if (!c || !joints) FAIL(c, RT_ERR_INVALID_ARG, "null argument");
    if (!c->scene_ready || mesh_index >= c->meshes.size()) FAIL(c, RT_ERR_INVALID_ARG, "bad mesh index");
    const MeshInfo& mi = c->meshes[mesh_index];
    if (!mi.skinned) FAIL(c, RT_ERR_INVALID_ARG, "mesh is not skinned");
    if (joint_count != mi.joint_count) FAIL(c, RT_ERR_INVALID_ARG, "joint count mismatch");
    HIPC(c, hipSetDevice(c->device));
    if (rt_status st = begin_update(c)) return st;   // frames in flight keep their generation
    Geo& g = c->G();
    float4 *pos = (float4*)g[Geo::pos].p + mi.vbase, *nrm = (float4*)g[Geo::nrm].p + mi.vbase;
    HIPC(c, hipMemcpyAsync(c->d_joints.p, joints, (size_t)joint_count * 64, hipMemcpyHostToDevice, c->ustream));
    // previousPositions <- positions (Renderer.swift:1290-1303)
    HIPC(c, hipMemcpyAsync((float4*)g[Geo::prev_pos].p + mi.vbase, pos, (size_t)mi.vcount * 16,
                           hipMemcpyDeviceToDevice, c->ustream));
    launch_skin((const float4*)c->d_rest_pos.p + mi.vbase, (const float4*)c->d_rest_nrm.p + mi.vbase,
                (const ushort4*)c->d_jidx.p + mi.vbase, (const float4*)c->d_jw.p + mi.vbase, (const float*)c->d_joints.p,
                pos, nrm, mi.vcount, c->ustream);
    launch_tri_nrm((const uint4*)c->d_tri_info.p, (const float4*)g[Geo::nrm].p, (float4*)g[Geo::tri_nrm].p, mi.tbase,
                   mi.tcount, c->ustream);
    HIPC(c, hipGetLastError());
    HIPC(c, hipStreamSynchronize(c->ustream));  // joint upload buffer is reused next call
    c->world_dirty = true;
    c->skin_moved = true;   // conservative: positions may now differ from previousPositions
    return RT_OK;
}

rt_status rt_debug_trace_host(const rt_scene_desc* sd, const float* rays, const float* tmax, uint32_t n, int32_t any,
                              float* t_out, uint32_t* id_out, float* u_out, float* v_out, uint32_t* nodes_out,
                              uint32_t* tris_out) {
    if (!sd || !rays || (n && (!t_out || !id_out))) FAIL((rt_ctx*)nullptr, RT_ERR_INVALID_ARG, "null argument");
    // world-space triangles in the original order, as rt_scene_upload makes them
    std::vector<float4> pos;
    std::vector<uint4> tri_info;
    std::vector<float> inst, world;
    flatten_scene(sd, pos, nullptr, tri_info, inst);
    world_tris(tri_info, pos, inst, world);
    const uint32_t nt = (uint32_t)tri_info.size();
    BvhResult bvh2;
    Bvh8Result bvh;
    if (!build_bvh8_fit(world.data(), nt, bvh2, bvh)) FAIL((rt_ctx*)nullptr, RT_ERR_UNSUPPORTED, "BVH too deep");
    const std::vector<float> tris = slot_ordered_tris(world, bvh.tri_order);
    DevScene S;
    std::memset(&S, 0, sizeof S);
    S.tris = tris.data();
    S.nodes8 = bvh.nodes.data();
    S.num_tris = (int)nt;
    S.num_nodes8 = (int)bvh.nodes.size();
    std::vector<int> stack((size_t)kStackSize * kBlock);
    for (uint32_t r = 0; r < n; ++r) {
        const float* q = rays + 6 * (size_t)r;
        f3 o = mk3(q[0], q[1], q[2]), d = mk3(q[3], q[4], q[5]);
        float tm = tmax ? tmax[r] : INFINITY;
        Hit h;
        TraceCounters tc{0, 0, 0};
        bool overflow = false;
        bool hit = any ? trace8<true, true>(S, o, d, 0.0f, tm, h, stack.data(), tc, overflow)
                       : trace8<false, true>(S, o, d, 0.0f, tm, h, stack.data(), tc, overflow);
        if (overflow) FAIL((rt_ctx*)nullptr, RT_ERR_STATE, "traversal stack overflow");
        t_out[r] = hit ? h.t : INFINITY;
        id_out[r] = hit ? h.id : 0xffffffffu;
        if (u_out) u_out[r] = hit ? h.u : 0.0f;
        if (v_out) v_out[r] = hit ? h.v : 0.0f;
        if (nodes_out) nodes_out[r] = tc.nodes;
        if (tris_out) tris_out[r] = tc.tris;
    }
    return RT_OK;
}

}  // extern "C"
