// rt_ctx.h — the context behind the C ABI (include/rt_api.h) and what the files that implement
// it share: rt_api.cpp (create / destroy, setters, statistics), rt_api_scene.cpp (scene, BVH,
// geometry updates), rt_api_frame.cpp (frames, reads, tiles, present), rt_api_query.cpp (device
// ray queries).  Internal.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <type_traits>
#include <vector>

#include "../../include/rt_api.h"
#include "rt_bvh.h"
#include "rt_frame_ring.h"
#include "rt_kernels.h"
#include "rt_wavefront.h"
#include "rt_resources.h"

struct MeshInfo {
    uint32_t vbase = 0, vcount = 0, joint_count = 0;
    uint32_t tbase = 0, tcount = 0;   // the mesh's triangles (original ids are assigned mesh by mesh)
    bool skinned = false;
};

// One frame in flight (Renderer.swift:207, 1406-1409 keeps up to 3): its wavefront memory, its
// per-frame targets and statistics, and the stream it renders on.  Consecutive frames rotate over
// the slots (rt::FrameRing) and overlap except where frame f needs frame f-1's results (the history
// target and the previous motion vectors: the extra-sample pass and the resolve).
struct FrameSlot {
    rt::DevBuf qc, qr, accum, meta, q0, q1, hits, sq, counts, extra, sorted, sort_table, sort_total, params;
    rt::DevBuf depth, gbuffer, counters;
    rt::DevBuf prim_hit;   // wavefront: per pixel, sample 0's last bounce-0 hit (id, u, v) for wf_motion
    // `wf` is passed to the kernels by value and stays plain: ensure_wavefront fills it in from the
    // buffers above and from the pinned blocks and events below, which own what it points to
    rt::WavefrontBuffers wf;
    rt::WfTimeline wft;
    rt::WfFrameStats wfs{};   // zero for a megakernel frame
    rt::Pinned<uint32_t> h_counts;           // wf.h_counts
    rt::Pinned<rt::FrameParams> h_params;    // wf.h_params; made last: set = the wavefront state is complete
    rt::Event wf_ev[std::extent<decltype(rt::WavefrontBuffers::ev)>::value];   // wf.ev
    rt::Event param_ev[rt::WavefrontBuffers::kParamSlots];                     // wf.param_ev
    rt::Event tl_ev[rt::WfTimeline::kMaxEv];                                   // wft.ev
    rt::Pinned<unsigned long long> h_counters;   // pinned copy of `counters` after the frame
    rt::Stream own_stream;                       // slots 1..; slot 0 renders on rt_ctx::stream
    rt::Event ev0, ev1, done;
    bool pending = false, wavefront = false;
    bool gbuf_written = false;                   // the slot's last frame wrote the G-buffer (enableDenoiseGBuffer)
    ~FrameSlot() {   // the frame graphs run_wavefront captured into the timeline
        for (hipGraphExec_t x : wft.exec)
            if (x) (void)hipGraphExecDestroy(x);
    }
};

// Per-frame geometry: what skinning, instance transforms and refit rewrite between frames, one
// copy per generation (rt::FrameRing; Renderer.swift keeps per-frame position buffers for the same
// reason, :1290-1303).  A new buffer is a new name before kCount.
struct Geo {
    enum Buf { pos, prev_pos, nrm, inst, prev_inst, tris, nodes, node_box, tri_bin, tri_nrm, root_box, kCount };
    rt::DevBuf buf[kCount];
    uint32_t num_nodes8 = 0;
    rt::DevBuf& operator[](Buf b) { return buf[b]; }
    const rt::DevBuf& operator[](Buf b) const { return buf[b]; }
};

// One device ray query in flight (rt_trace_closest / rt_trace_any / rt_resolve_hits / rt_shade_hits /
// the path queries): the launch's
// own device state (chunk counters and statistics, rt_kernels.h RqParams::state), its pinned copy and its events.
// Queries rotate over kQuerySlots of these, so launches that may overlap (other streams) share no
// counter; a slot is reused once its previous query has finished (harvest_query).
constexpr int kQuerySlots = 4;
struct QuerySlot {
    rt::DevBuf state;
    rt::DevBuf scratch;         // rt_compact_paths: the call's selection words and tile counts (rt_paths.h); grown on demand
    rt::Pinned<unsigned long long> h_counters;
    rt::Event ev0, ev1, done;   // around the launch (timing); after the counters' copy
    bool pending = false, any = false;
    bool counted = false;       // a trace: folded into rt_query_stats; every other query uses `done` only
    uint32_t blocks = 0;        // the launch's grid
};

struct rt_ctx {
    int device = 0;
    int pipeline = RT_PIPELINE_MEGAKERNEL;
    int tail_paths = 0;
    int sort_bins = rt::kSortBinsDefault;   // 0 = no hit sort
    rt::Stream own_stream;
    hipStream_t stream = nullptr;    // own_stream, or the caller's (rt_set_stream)
    std::string err;
    bool counting = false;
    bool spans = false;              // rt_set_device_spans
    bool graphs = true;              // rt_set_graphs
    rt_tuning tuning_req{};          // rt_set_tuning as given (0 = default)
    rt::WfTuning tuning;             // ... resolved

    // host scene copies
    std::vector<float4> h_pos, h_nrm;
    std::vector<uint4> h_tri_info;
    std::vector<float> h_inst;
    std::vector<Material> h_mat;
    std::vector<Light> h_lights;
    std::vector<MeshInfo> meshes;
    std::vector<float> h_world;   // 9 floats per triangle
    int max_sub = 1;
    uint32_t num_tris = 0, num_verts = 0, num_inst = 0;
    bool scene_ready = false, bvh_ready = false;
    bool world_dirty = false;  // device positions/transforms changed since h_world was computed

    // BVH
    rt::BvhResult bvh;
    rt::Bvh8Result bvh8;
    std::vector<uint32_t> level_nodes;
    std::vector<uint32_t> level_off;

    // device buffers; dev_bytes is their running size (dev_alloc / dev_free)
    size_t dev_bytes = 0;
    Geo geo[rt::kGens];
    rt::Stream ustream;              // geometry updates (skin, transforms, refit)
    rt::Event uev;                   // end of the latest update batch; frames wait on it
    bool uev_valid = false;
    Geo& G() { return geo[ring.write_gen()]; }   // the generation updates and builds write
    rt::DevBuf d_rest_pos, d_rest_nrm, d_jidx, d_jw, d_joints;
    rt::DevBuf d_tri_info, d_mat, d_lights, d_halton;
    rt::DevBuf d_tex_texels, d_tex_info, d_mat_tex, d_uv, d_tex_lut;   // texture path (textured scenes)
    bool textured = false;
    rt::DevBuf d_slot_to_tri, d_levels, d_maxabs, d_lbvh_scratch;
    uint32_t num_nodes8 = 0;
    rt::Pinned<uint32_t> h_lbvh;   // pinned word for the device builder's level counts
    // tree quality under refit (rt_tuning.refit_rebuild_pct): the node-area sum (launch_bvh_cost)
    // of the last build and of the last refit (rt_stats.bvh_cost_*), the latter read back
    // asynchronously
    rt::DevBuf d_cost;
    rt::Pinned<float> h_cost;
    rt::Event cost_ev;
    bool cost_pending = false;
    rt::DevBuf d_random, d_accum[2];       // accum[ring.read_idx] = history (TextureIndexAccumulation)
    rt::DevBuf d_motion[rt::kMotionTargets];
    int width = 0, height = 0;
    uint32_t last_frame_index = 0;   // Uniforms.frameIndex of the newest frame
    // display output (rt_present): temporal-scaler history at the output size, sRGB thresholds
    rt::DevBuf d_hist[2], d_hdepth[2], d_present_out, d_present_thr;
    rt::DevBuf d_half;   // rt_read_radiance_half staging (RGBA16F)
    int hist_w = 0, hist_h = 0, hist_idx = 0;
    bool hist_valid = false;
    rt::DevBuf d_den[4];   // RT_SCALER_DENOISED scratch at render size: ping, pong, guide, albedo
    size_t den_n = 0;
    rt_stats stats{};      // the last frame's fields and the running totals (harvest)

    // frames in flight
    FrameSlot slot[rt::kMaxSlots];
    rt::FrameRing ring;
    int max_in_flight = 0;           // rt_opts.frames_in_flight; 0 = by frame size (wf_in_flight)
    rt::Event scene_ev;              // ctx->stream work a slot-1.. frame must follow

    // device ray queries (rt_api_query.cpp)
    QuerySlot qslot[kQuerySlots];
    int qnext = 0;                   // the slot the next query takes (the oldest)
    rt::DevBuf d_sub_first;          // first scene-wide triangle id per [mesh * max_sub + submesh]
    size_t q_scratch_max = 0;        // the largest compaction scratch asked for: a slot that grows grows to this
    rt::Event q_uev;                 // the update stream's state a query's stream waits for
    rt_query_stats qstats{};
    bool q_overflow = false;         // a harvested query overflowed its stack: reported by rt_wait / rt_get_query_stats

    // motion bookkeeping for the extra-sample pass: motion vectors are exactly zero unless the
    // camera, an instance transform or skinned positions differ from their previous copies
    bool inst_moved = false, skin_moved = false, last_moving = false;
};

extern thread_local std::string rt_g_err;   // rt_last_error(NULL)

#define FAIL(ctx, code, msg)                 \
    do {                                     \
        if (ctx) (ctx)->err = (msg);         \
        rt_g_err = (msg);                    \
        return (code);                       \
    } while (0)

#define HIPC(ctx, expr)                                                                            \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess) {                                                                    \
            std::string m_ = std::string(#expr) + ": " + hipGetErrorString(e_);                    \
            if (ctx) (ctx)->err = m_;                                                              \
            rt_g_err = m_;                                                                         \
            return e_ == hipErrorOutOfMemory ? RT_ERR_OUT_OF_MEMORY : RT_ERR_HIP;                  \
        }                                                                                          \
    } while (0)

// rt_api.cpp.  dev_alloc keeps a buffer that is large enough, else frees and reallocates it; zero
// bytes free it.  dev_upload without a stream copies on ctx->stream (and counts as work frames follow).
rt_status dev_alloc(rt_ctx* c, rt::DevBuf& b, size_t bytes);
rt_status dev_upload(rt_ctx* c, rt::DevBuf& b, const void* src, size_t bytes, hipStream_t s = nullptr);
inline void dev_free(rt_ctx* c, rt::DevBuf& b) { b.release(c->dev_bytes); }
int refit_rebuild_pct(const rt_ctx* c);   // rt_tuning.refit_rebuild_pct with its default
// rt_api_frame.cpp: waits for every frame in flight
rt_status drain_frames(rt_ctx* c);
// rt_api_query.cpp: waits for every pending query and folds it into rt_query_stats, oldest first.
// Everything that writes geometry or the tree calls it first, so no query races an update of the
// generation it reads; rt_wait and rt_get_query_stats report a stack overflow it found.
rt_status drain_queries(rt_ctx* c);
// rt_api_scene.cpp: rebuilds the tree once a refit has degraded it (before a refit or a frame)
rt_status check_refit_quality(rt_ctx* c, bool* rebuilt);
