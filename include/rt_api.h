/*
 * rt_api.h — C-ABI of the MI355X path-tracer hot path (librt_hip.so).
 *
 * This is the drop-in boundary for the reference's one GPU hot path, the Metal compute kernel
 * `raytracingKernel` (MetalRaytracing/Raytracing.metal:220-831) and the host code that binds and
 * dispatches it.  Each entry point names the reference interface it replaces:
 *
 *   rt_create / rt_destroy     Renderer.init?(metalView:) device+queue+pipeline setup
 *                              (Renderer.swift:228-341), deinit
 *   rt_scene_upload            createBuffers: Resource argument buffer, material buffers,
 *                              vertex/index buffers, light buffer (Renderer.swift:342-420,
 *                              SubMesh.swift:38-54, Scene.swift:93)
 *   rt_bvh_build               createMTL4AccelerationStructures BLAS+TLAS build
 *                              (Renderer.swift:464-606, Utilities.swift:101-290)
 *   rt_bvh_build_device        the same build on the GPU (LBVH + 8-wide collapse); also the
 *                              legacy full rebuild of a deformed scene (Renderer.swift:1252-1277)
 *   rt_set_instance_transforms updateInstanceDescriptors (Renderer.swift:937-973): current ->
 *                              previous copy, then new transforms
 *   rt_skin                    SkinningPass.dispatchSkinning + prev-position copy
 *                              (SkinningPass.swift:160-211, Renderer.swift:1290-1310)
 *   rt_bvh_refit               refitMTL4AccelerationStructures (Renderer.swift:1084-1202)
 *   rt_resize                  createTextures: accumulation ping-pong, random-offset texture,
 *                              depth/motion/G-buffer targets (Renderer.swift:676-804)
 *   rt_render_frame            Renderer.draw: argument-table binding + 16x16 dispatch of
 *                              raytracingKernel + ping-pong swap (Renderer.swift:1405-1503)
 *   rt_trace_closest/rt_trace_any  `intersector.intersect` called from any other kernel: batches
 *                              of the caller's rays against the built scene
 *   rt_resolve_hits / rt_shade_hits  what such a kernel does with the hit: the Resource-buffer
 *                              reads (:324-456) and the shading up to the next ray (:517-774)
 *   rt_*_indirect              the same queries with their record count read from device memory
 *                              (indirect dispatch: a compaction's count feeds the next launch)
 *   rt_read_radiance/rt_read_aux  (no reference equivalent: the reference never reads back;
 *                              replaces presenting dstTex/depthTex/motionTex to MetalFX)
 *
 * Conventions: every function returns rt_status (0 = OK); rt_last_error(ctx) describes the last
 * failure.  No exceptions or aborts cross this boundary.  The caller owns every host array and
 * may free it once the call returns.  One context per GPU, used from one host thread.  All
 * work is issued on one HIP stream per context (rt_set_stream may substitute the caller's).
 */
#ifndef RT_API_H
#define RT_API_H

#include "rt_types.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef int32_t rt_status;
#define RT_OK 0
#define RT_ERR_INVALID_ARG 1
#define RT_ERR_HIP 2
#define RT_ERR_IO 3
#define RT_ERR_OUT_OF_MEMORY 4
#define RT_ERR_STATE 5
#define RT_ERR_UNSUPPORTED 6
#define RT_ERR_NO_DEVICE 7

typedef struct rt_ctx rt_ctx;

/* ---- scene description (caller-owned, copied by rt_scene_upload) ------------------------- */

/* A decoded texture (the MTLTexture of SubMesh.swift:69-241): width x height RGBA8 texels,
 * row-major, row 0 = the image's top row (texcoord v = 0 after the shader's flip,
 * Raytracing.metal:416).  Base color and emission slots decode sRGB, the others are linear
 * (the loader options of SubMesh.swift:80-97). */
typedef struct rt_texture_desc {
    const uint8_t* rgba8;
    uint32_t width;
    uint32_t height;
} rt_texture_desc;

/* Texture slot k of a submesh <-> MATERIAL_TEXTURE_* bit k of its material's textureFlags:
 * 0 base color, 1 tangent-space normal, 2 roughness, 3 metallic, 4 AO, 5 emission, 6 opacity. */
#define RT_TEXTURE_SLOTS 7

/* One Submesh: a material group of one mesh (SubMesh.swift:18-54). Indices are u32
 * (u16 assets are widened, SubMesh.swift:243-265), three per triangle.  textures[k]: index into
 * rt_scene_desc.textures for every slot whose bit is set in material.textureFlags (other
 * entries are ignored); the AO slot is not sampled (ENABLE_AO = 0, ShaderTypes.h:155-156). */
typedef struct rt_submesh_desc {
    const uint32_t* indices;
    uint32_t index_count;
    uint32_t _pad;
    Material material;
    int32_t textures[8];
} rt_submesh_desc;

/* One Mesh = one instance of the two-level acceleration structure (Mesh.swift:17-68). Vertex
 * streams follow Model.vertexDescriptor (Model.swift:304-341): positions and normals float3 at
 * a 16-byte stride, uvs float2 (may be NULL), joint indices ushort4 and weights float4 (NULL
 * unless skinned).  `transform` is the object->world MTLPackedFloat4x3 of the instance
 * descriptor (Renderer.swift:547-556). */
typedef struct rt_mesh_desc {
    const rt_float3* positions;
    const rt_float3* normals;
    const rt_float2* uvs;
    const uint16_t* joint_indices;
    const float* joint_weights;
    uint32_t vertex_count;
    uint32_t submesh_count;
    const rt_submesh_desc* submeshes;
    rt_packed_float4x3 transform;
    uint32_t joint_count;   /* > 0: skinned mesh (rt_skin rewrites its positions/normals) */
    uint32_t _pad;
} rt_mesh_desc;

typedef struct rt_scene_desc {
    uint32_t mesh_count;
    uint32_t light_count;
    const rt_mesh_desc* meshes;
    const Light* lights;
    uint32_t texture_count;
    uint32_t _pad;
    const rt_texture_desc* textures;
} rt_scene_desc;

/* ---- context ------------------------------------------------------------------------------- */

#define RT_PIPELINE_MEGAKERNEL 0  /* one thread per pixel, the reference's kernel shape */
#define RT_PIPELINE_WAVEFRONT 1   /* generate / extend / shade / connect / resolve queues */

typedef struct rt_opts {
    int32_t device;     /* HIP device ordinal */
    int32_t pipeline;   /* RT_PIPELINE_* */
    int32_t tail_paths; /* wavefront: below this many live paths the rest of the frame runs in the
                           persistent finish kernel; 0 = default (4194304 one frame at a time,
                           1310720 / 1048576 / 786432 / 524288 with 2 / 3 / 4 / 5+ frames in flight), 1 = never */
    int32_t sort_bins;  /* wavefront: hits are sorted into this many bins of BVH leaf order between
                           extend and shade (a power of two in [1024, 4096]); 0 = default (no
                           sort), < 0 = no sort.  Never changes the image, only memory locality. */
    int32_t frames_in_flight; /* wavefront on the context's own stream: frames rendered concurrently,
                                 each overlapping the previous one until it needs that frame's
                                 accumulation / motion output; 0 = default (one per hardware
                                 queue: 8 when the process has GPU_MAX_HW_QUEUES >= 8, 4
                                 otherwise, as many as fit in 96 GB, at least 2), 1 = one at a
                                 time, at most 8.  Each slot holds ~300 B per allocated path,
                                 pixels x (spp + extra samples).  With four or
                                 more slots the finish tail takes 20 % of the resident grid,
                                 with two 40 %.
                                 Geometry updates (skinning, transforms, refit, builds) rotate
                                 over max(2, frames in flight) generations, so per-frame updates
                                 keep every slot's overlap.  Images are identical either way. */
    int32_t reserved[3];
} rt_opts;

/* Image-space tile partition for multi-GPU rendering: the image is cut into
 * tile_size x tile_size tiles numbered row-major; this rank renders tiles with
 * tile_id % nranks == rank.  A NULL tile set (or nranks <= 1) renders the whole image. */
typedef struct rt_tile_set {
    int32_t tile_size;
    int32_t rank;
    int32_t nranks;
    int32_t _pad;
} rt_tile_set;

typedef struct rt_stats {
    uint64_t closest_rays;  /* closest-hit queries traced in the last frame (incl. primary) */
    uint64_t shadow_rays;   /* any-hit shadow queries traced in the last frame */
    uint64_t node_visits;   /* BVH node tests (counting frames only, see rt_set_counting) */
    uint64_t tri_tests;     /* triangles tested (counting frames only) */
    uint64_t paths;         /* pixel samples started */
    uint64_t bvh_nodes;     /* nodes in the current BVH */
    uint64_t triangles;     /* triangles in the current scene */
    uint64_t device_bytes;  /* device memory held by the context */
    float last_frame_ms;    /* device time of the last rt_render_frame (HIP events) */
    float kernel_ms[7];     /* per-stage device time of the last frame: megakernel [0];
                               wavefront [0] generate [1] extend [2] shade [3] connect [4] resolve
                               [5] finish (tail) [6] hit sort */
    int32_t pipeline;       /* RT_PIPELINE_* that rendered the last frame */
    int32_t iterations;     /* wavefront: extend/shade/connect rounds of the last frame */
    /* wavefront: the queue traversal kernel (extend + connect launches; the finish tail excluded) */
    uint64_t trace_rays;    /* rays it traced */
    uint64_t trace_nodes;   /* nodes it fetched (counting frames only) */
    uint64_t trace_tris;    /* triangles it tested (counting frames only) */
    int32_t trace_launches; /* its launches */
    float trace_ms;         /* its summed device time (HIP events on the render stream) */
    uint64_t trace_closest_rays; /* the closest-hit (extend) share of trace_rays */
    int32_t finish_launches;     /* wavefront: persistent finish launches (their time: kernel_ms[5]) */
    int32_t frames_in_flight;    /* frames the last rt_render_frame could overlap (1..8) */
    /* running totals over every finished frame since rt_create (frames submitted back to back
       without rt_wait are each counted) */
    uint64_t frames_total;
    uint64_t total_closest_rays;
    uint64_t total_shadow_rays;
    uint64_t total_paths;
    double total_frame_ms;         /* sum of last_frame_ms */
    double total_kernel_ms[7];     /* sums of kernel_ms */
    uint64_t total_trace_rays;     /* sums of trace_rays, trace_closest_rays, trace_ms, trace_launches, */
    uint64_t total_trace_closest_rays;   /* finish_launches */
    double total_trace_ms;
    uint64_t total_trace_launches;
    uint64_t total_finish_launches;
    /* reserved, always 0 (node visits served from an LDS copy of the BVH's top levels: that
       staging was measured and removed) */
    uint64_t node_visits_lds;
    uint64_t trace_nodes_lds;
    /* wavefront, device clock: each launch from its first workgroup's start to its last wave's end
       (s_memrealtime, 100 MHz), what a kernel trace records for a dispatch.  With frames in flight
       the HIP events of trace_ms / kernel_ms also count the time a launch waits for CUs that other
       frames' kernels hold. */
    float trace_dev_ms;            /* extend + connect launches of the last frame */
    int32_t trace_dev_launches;
    float finish_dev_ms;           /* finish launches of the last frame */
    int32_t finish_dev_launches;
    double total_trace_dev_ms;     /* running sums of the four above */
    uint64_t total_trace_dev_launches;
    double total_finish_dev_ms;
    uint64_t total_finish_dev_launches;
    /* wavefront frames (device-driven, the default) by how they were submitted (running totals):
       replayed from the slot's two captured HIP graphs, captured anew and launched (first frame of
       a slot, or a launch argument changed), enqueued eagerly because the runtime refused a
       capture (the slot then stays eager), enqueued eagerly by choice (RT_GRAPH=0, host-driven
       rounds).  The replacement of the reference's per-frame command buffers
       (Renderer.swift:1405-1490). */
    uint64_t total_graph_replays;
    uint64_t total_graph_captures;
    uint64_t total_graph_fallbacks;
    uint64_t total_graph_eager;
    /* tree quality (rt_tuning.refit_rebuild_pct): device rebuilds a degraded refit triggered, and the
       node-area sum (the sum of the 8-wide node boxes' areas: the SAH node term, proportional to the
       node visits of the scene's rays) of the last build and of the last refit read back (0 before
       the first refit; a rebuild leaves the refit figure that triggered it) */
    uint64_t total_auto_rebuilds;
    float bvh_cost_built;
    float bvh_cost_refit;
    /* closest-hit rays their producer retired: the exact boxes of the BVH root's children proved a
       miss (root mask 0), so the ray was never enqueued.  They count in closest_rays, trace_rays and
       trace_closest_rays as the misses wf_trace would have resolved.  Last frame; running total. */
    uint64_t root_retired_rays;
    uint64_t total_root_retired_rays;
    /* shadow rays a shading step resolved without a traversal; each counts in shadow_rays, and those
       the wavefront's shade stage resolved in trace_rays, as the rays its connect launch would have
       traced.  dark: the contribution is ±0 in every component, so the answer cannot change the
       radiance (either pipeline).  root_unoccluded: the exact boxes of the BVH root's children
       proved the ray unoccluded (root mask 0) and the shade stage added its contribution
       (wavefront).  Last frame; running totals. */
    uint64_t dark_shadow_rays;
    uint64_t root_unoccluded_shadow_rays;
    uint64_t total_dark_shadow_rays;
    uint64_t total_root_unoccluded_shadow_rays;
} rt_stats;

rt_status rt_create(const rt_opts* opts, rt_ctx** out);
rt_status rt_destroy(rt_ctx* ctx);
const char* rt_last_error(const rt_ctx* ctx);   /* ctx may be NULL: last global error */
rt_status rt_set_stream(rt_ctx* ctx, void* hip_stream);  /* NULL restores the own stream */

rt_status rt_scene_upload(rt_ctx* ctx, const rt_scene_desc* scene);
rt_status rt_bvh_build(rt_ctx* ctx);
/* On-device build from the uploaded (and possibly skinned / re-transformed) geometry: Morton
 * sort + radix tree + top-down collapse into the same 8-wide layout.  Milliseconds instead of the
 * host SAH build's seconds; traversal visits more nodes per ray (LBVH quality).  Images are
 * identical to those of a host-built tree (conservative boxes).  Fails with
 * RT_ERR_UNSUPPORTED when the tree is deeper than the traversal stack. */
rt_status rt_bvh_build_device(rt_ctx* ctx);
rt_status rt_bvh_refit(rt_ctx* ctx);
rt_status rt_set_instance_transforms(rt_ctx* ctx, const rt_packed_float4x3* transforms, uint32_t count);
/* Linear-blend skinning of one skinned mesh (Skinning.metal:7-49). `joint_matrices` are
 * column-major float4x4 (host memory). Copies current positions to previous first. */
rt_status rt_skin(rt_ctx* ctx, uint32_t mesh_index, const float* joint_matrices, uint32_t joint_count);

/* (Re)create the per-pixel targets; `random_offsets` is W*H uint32 (row-major). Resets history. */
rt_status rt_resize(rt_ctx* ctx, int32_t width, int32_t height, const uint32_t* random_offsets);

/* Render one frame (asynchronous; rt_wait to block). Reads the history written by the previous
 * call, writes the new accumulation and swaps (Renderer.swift:1492-1494). */
rt_status rt_render_frame(rt_ctx* ctx, const Uniforms* uniforms, const rt_tile_set* tiles);
rt_status rt_wait(rt_ctx* ctx);

/* Copies of the latest outputs into caller host memory: radiance RGBA float32 W*H*4 (the
 * accumulation target just written; the reference stores it as RGBA16F), depth W*H,
 * motion W*H*2 (pixels, +Y down), G-buffer 4 planes of W*H*4 (diffuse, specular, normal,
 * roughness) or NULL. Rows are in the kernel's tid.y order (row 0 = bottom of the view). */
rt_status rt_read_radiance(rt_ctx* ctx, float* rgba);
/* The same radiance as RGBA16F (uint16_t bit patterns, W*H*4), the format the reference's
 * accumulation texture holds (Renderer.swift:685, Raytracing.metal:819): the fp32 target rounded
 * to nearest even on the device (overflow to infinity, fp16 denormals kept); 8 B per pixel read
 * back instead of 16. */
rt_status rt_read_radiance_half(rt_ctx* ctx, uint16_t* rgba);
rt_status rt_read_aux(rt_ctx* ctx, float* depth, float* motion, float* gbuffer);

/* Display output (FramePresenter.swift:103-238, Shaders.metal:39-52): the newest radiance,
 * resampled to out_width x out_height by `scaler`, tone-mapped color / (1 + color) and encoded
 * to 8-bit RGBA rows top-down (alpha 255), written to host memory.  RT_SCALER_NONE samples the
 * nearest render pixel (the presenter's own path); SPATIAL resamples bilinearly; TEMPORAL blends
 * with the previous output reprojected through the motion vectors, clamped to the current
 * neighbourhood, rejected on depth jumps (MetalFX's scalers are unpublished: these are stand-ins
 * consuming the same inputs).  DENOISED (MTLFXTemporalDenoisedScaler's place when
 * useTemporalDenoiser is set, FramePresenter.swift:77-98,179-198) first filters the radiance at
 * render size, guided by the G-buffer (enableDenoiseGBuffer must be on: RT_ERR_STATE otherwise):
 * demodulation by diffuse + specular albedo, `denoise_passes` edge-avoiding a-trous passes over
 * normals and depth, remodulation; then the TEMPORAL path.  DENOISED and TEMPORAL share one
 * history.  encode: RT_ENCODE_SRGB8 (default) or RT_ENCODE_LINEAR8. */
#define RT_SCALER_NONE 0
#define RT_SCALER_SPATIAL 1
#define RT_SCALER_TEMPORAL 2
#define RT_SCALER_DENOISED 3
#define RT_ENCODE_SRGB8 0
#define RT_ENCODE_LINEAR8 1
typedef struct rt_present_opts {
    int32_t out_width;   /* 0 = render width */
    int32_t out_height;  /* 0 = render height */
    int32_t scaler;
    int32_t encode;
    int32_t denoise_passes;   /* RT_SCALER_DENOISED: 0 = 3; at most 6 */
    int32_t reserved[3];
} rt_present_opts;
rt_status rt_present(rt_ctx* ctx, const rt_present_opts* opts, uint8_t* host_rgba8);

/* Multi-GPU: pack this rank's tiles of the latest radiance into a device buffer of
 * rt_tile_count(...) * tile_size^2 * 4 floats, and the inverse on the gathering rank
 * (writing into the latest radiance target). Device pointers; enqueued after the newest frame
 * on the ctx stream (the _on forms: on `hip_stream` exactly as given, e.g. the stream the
 * collective runs on; NULL is HIP's null stream, PyTorch's default stream), without a host wait.  The next frames overlap them (see frames_in_flight); rt_wait waits for
 * them too. */
int32_t rt_tile_count(int32_t width, int32_t height, const rt_tile_set* tiles);
rt_status rt_pack_tiles(rt_ctx* ctx, const rt_tile_set* tiles, void* device_dst);
rt_status rt_unpack_tiles(rt_ctx* ctx, const rt_tile_set* tiles, const void* device_src);
rt_status rt_pack_tiles_on(rt_ctx* ctx, const rt_tile_set* tiles, void* device_dst, void* hip_stream);
rt_status rt_unpack_tiles_on(rt_ctx* ctx, const rt_tile_set* tiles, const void* device_src, void* hip_stream);
/* Host-memory forms of the same layout (RGBA fp32 images of width x height), for gathers that
 * land in host memory and for tests of the tile protocol without a device. */
rt_status rt_pack_tiles_host(int32_t width, int32_t height, const rt_tile_set* tiles, const float* src_rgba,
                             float* dst_packed);
rt_status rt_unpack_tiles_host(int32_t width, int32_t height, const rt_tile_set* tiles, const float* src_packed,
                               float* dst_rgba);

/* Device ray/node counters: when enabled, frames also count BVH node visits / triangle tests
 * (a few percent slower). Ray counts are always collected. */
rt_status rt_set_counting(rt_ctx* ctx, int32_t enabled);
/* Device-clock launch spans of the wavefront traversal and finish launches (rt_stats
 * total_*_dev_ms; block 0's start to the last wave's end, s_memrealtime), for frames submitted
 * while enabled.  Off by default: the stamps cost ~1 % of a C3g frame.  Measurement only (no
 * reference counterpart). */
rt_status rt_set_device_spans(rt_ctx* ctx, int32_t enabled);
/* Wavefront frames captured once per frame slot as HIP graphs and replayed (default: on), or
 * enqueued launch by launch (off) — the
 * replacement of the reference's per-frame command buffers (Renderer.swift:1405-1490).  Under a
 * HIP runtime that takes no timing events inside a graph, replayed frames record no per-stage
 * times (rt_stats kernel_ms); frames submitted with graphs off always do. */
rt_status rt_set_graphs(rt_ctx* ctx, int32_t enabled);
rt_status rt_get_stats(rt_ctx* ctx, rt_stats* out);

/* Scheduling parameters of the wavefront kernels (no reference counterpart: the
 * Metal driver schedules the reference's one kernel).  0 in any field selects the measured default;
 * images are identical for every value.  The library reads no environment variable
 * for these: only this call changes them, per context.  rt_set_tuning(ctx, NULL) restores the
 * defaults; a field outside its stated range is RT_ERR_INVALID_ARG.  rt_get_tuning returns the
 * values in effect for the fields with a fixed default; team, finish_grid_pct and trace_grid_pct
 * read back 0 when left at their default, which is chosen per frame from the frame size and the
 * frames in flight (rt_stats reports the frame's rounds and launches, not these choices). */
typedef struct rt_tuning {
    int32_t trace_chunk;        /* rays per chunk grab of the bulk traversal launches (default 64; <= 4096) */
    int32_t finish_chunk;       /* paths per chunk grab of the finish launch (default 64; <= 4096) */
    int32_t refill_min;         /* traversal / finish waves refill once this many lanes are idle (default 8) */
    int32_t shade_min;          /* the finish kernel shades once this many lanes wait for it (default 24) */
    int32_t shade_min_drained;  /* the same once its queue has run out: > 0 lanes, < 0 that percentage of
                                   the wave's busy lanes (default -50) */
    int32_t team;               /* finish drain, lanes per query once a wave holds <= 64 / team paths:
                                   0 = default (4 for frames of 256K .. 2.5M base paths, else off),
                                   1 = off, 2 / 4 / 8 */
    int32_t finish_grid_pct;    /* percent of the resident grid the finish launch takes (default by
                                   frames in flight: 100 / 40 / 33 / 20 for 1 / 2 / 3 / 4+) */
    int32_t trace_grid_pct;     /* percent of the resident grid the bulk traversal launches take
                                   (default 100; 60 with four to seven frames in flight; with eight,
                                   20 / 30 / 40 for frames of up to 2.5M / 6M / more base paths) */
    int32_t shade_blocks;       /* wf_shade grid, a multiple of 8 (default 2048; <= 65536) */
    int32_t host_rounds;        /* 1: host-driven rounds (each round's queue size read back); default 0:
                                   device-side round control, whole frames as HIP graphs */
    int32_t log;                /* 1: per-round queue sizes, stage times and finish diagnostics on stderr
                                   (host-driven rounds); 2: + per-path segment counts (slower) */
    int32_t device_bvh;         /* rt_bvh_build_device topology: 0 = PLOC clustering (default),
                                   1 = LBVH radix tree */
    int32_t refit_rebuild_pct;  /* rt_bvh_refit keeps the topology and grows the boxes of moved
                                   geometry; once a refit's node-area sum (rt_stats.bvh_cost_refit)
                                   exceeds this percentage of the last build's, the next
                                   rt_bvh_refit or rt_render_frame rebuilds the tree on the device
                                   (rt_bvh_build_device) instead.  0 = default (150), < 0 = never.
                                   Images are the same either way. */
    int32_t reserved[3];
} rt_tuning;
rt_status rt_set_tuning(rt_ctx* ctx, const rt_tuning* tuning);
rt_status rt_get_tuning(const rt_ctx* ctx, rt_tuning* out);

/* ---- device ray queries ---------------------------------------------------------------------
 * The reference's `intersector.intersect` outside raytracingKernel (any Metal kernel may call
 * it): trace a batch of the caller's rays against the built scene on the GPU.  `rays`, `hits`
 * and `occluded` are DEVICE pointers; the calls enqueue one kernel launch and return without a
 * host wait (results are ordered on the stream the query ran on; rt_wait waits for them too).
 *
 * Both records are 32 B, 16-byte aligned, and read / written as two 16-B words. */
typedef struct rt_ray {      /* 32 B */
    float origin[3];
    float reserved;          /* ignored */
    float direction[3];      /* need not be unit length; t is in units of it */
    float tmax;              /* hits with t in [0, tmax]; INFINITY = unbounded */
} rt_ray;

#define RT_MISS 0xffffffffu
typedef struct rt_ray_hit {  /* 32 B */
    float t;                 /* INFINITY on a miss */
    float u, v;              /* barycentrics in the library's convention (u -> v1, v -> v2); 0 on a miss */
    uint32_t triangle;       /* scene-wide triangle id (meshes, then submeshes, in upload order); RT_MISS */
    uint32_t mesh;           /* instance_id of Metal's intersection result; RT_MISS */
    uint32_t submesh;        /* geometry_id; RT_MISS */
    uint32_t primitive;      /* primitive_id: triangle index within the submesh; RT_MISS */
    uint32_t reserved;       /* 0 */
} rt_ray_hit;

/* The last query's figures and the running totals since rt_create (a separate struct: rt_stats
 * keeps its layout).  Node visits and triangle tests are counted only by queries enqueued while
 * rt_set_counting is on. */
typedef struct rt_query_stats {
    uint64_t rays;           /* rays of the last query */
    uint64_t hits;           /* closest-hit: rays that hit; any-hit: occluded rays */
    uint64_t node_visits;
    uint64_t tri_tests;
    uint32_t grid_blocks;    /* blocks of 256 threads the launch took */
    int32_t any_hit;         /* the last query was rt_trace_any */
    float device_ms;         /* device time of the launch (HIP events around it) */
    uint32_t reserved;
    uint64_t queries_total;  /* queries launched (n > 0) */
    uint64_t total_rays;
    uint64_t total_hits;
    uint64_t total_node_visits;
    uint64_t total_tri_tests;
    uint64_t total_grid_blocks;
    double total_device_ms;
} rt_query_stats;

/* Semantics:
 *  - Closest hit follows the renderer's rule: nearest t, ties to the lower triangle id.  The result
 *    is independent of which builder made the tree and bit-identical to rt_debug_trace_host on the
 *    same geometry.  Any hit reports occlusion only (1 / 0 per ray): which occluder is found
 *    depends on the tree, so none is returned.
 *  - Geometry seen: exactly what the next rt_render_frame would see, i.e. the newest committed
 *    geometry generation; the query's stream first waits for the update stream (skinning,
 *    transforms, refit enqueued before the call).
 *  - No race with updates: rt_skin, rt_set_instance_transforms, rt_bvh_refit, both builds, the
 *    automatic rebuild and rt_scene_upload first wait, on the host, for every pending query.
 *  - rt_wait and rt_destroy wait for queries too.  Frames share nothing writable with queries:
 *    frames rendered with queries interleaved are bit-identical to frames rendered without.
 *  - Back-to-back queries, also on different streams, need no host wait between them: each
 *    launch owns one of a small ring of device states (chunk counters, statistics); a state is
 *    reused only once its previous query has finished.
 *  - Needs only the scene and a BVH (either pipeline; no rt_resize).
 *  - The plain forms run on the context's stream, the _on forms on `hip_stream` exactly as
 *    given (NULL is HIP's null stream), as rt_pack_tiles / rt_pack_tiles_on do.
 *  - Errors: a NULL pointer with n > 0, or a pointer not 16-byte aligned (4-byte for
 *    `occluded`): RT_ERR_INVALID_ARG.  Before a BVH build: RT_ERR_STATE.  n == 0: RT_OK, nothing
 *    is launched.  A traversal-stack overflow is counted on the device and returned as
 *    RT_ERR_STATE by the next rt_wait or rt_get_query_stats, as frames report theirs.
 *  - rt_get_query_stats waits for pending queries before it reads. */
rt_status rt_trace_closest(rt_ctx* ctx, const rt_ray* rays, uint32_t n, rt_ray_hit* hits);
rt_status rt_trace_any(rt_ctx* ctx, const rt_ray* rays, uint32_t n, uint32_t* occluded);
rt_status rt_trace_closest_on(rt_ctx* ctx, const rt_ray* rays, uint32_t n, rt_ray_hit* hits, void* hip_stream);
rt_status rt_trace_any_on(rt_ctx* ctx, const rt_ray* rays, uint32_t n, uint32_t* occluded, void* hip_stream);
rt_status rt_get_query_stats(rt_ctx* ctx, rt_query_stats* out);

/* ---- Surface queries: a ray and its hit record resolved into shading inputs ---------------------
 * What a Metal kernel does after `intersector.intersect`: read the Resource buffers for the vertex
 * normals, the UVs, the instance matrix, the material and its maps (Raytracing.metal:324-339,
 * :391-456, :492-504).  Here those buffers are the library's, in its own layouts, so the library
 * resolves the hit: rt_resolve_hits turns `n` rays (the ones that were traced) and their
 * rt_ray_hit records into one rt_surface and, unless `materials` is NULL, one
 * rt_surface_material each.  Every float is the one the renderer's own shading forms at that hit,
 * bit for bit (the same expressions in the same order; with the G-buffer on, a frame's normal,
 * albedo and roughness planes equal the records of its sample-0 primary rays).  With
 * rt_trace_closest, the caller's own ray generation and rt_trace_any this is a complete
 * user-side integrator (ambient occlusion, lidar, visibility baking).
 *
 * `rays`, `hits`, `surfaces` and `materials` are DEVICE pointers; the call enqueues one kernel
 * launch (one thread per record, no host wait).  rt_surface is 64 B and written as four 16-B
 * words, rt_surface_material 48 B as three. */
typedef struct rt_surface {          /* 64 B */
    float position[3];       /* origin + direction * t (the renderer's P, :336) */
    float t;                 /* copied from the hit */
    float normal[3];         /* the renderer's Ng: the interpolated vertex normal through the instance
                                4x3, normalised; -direction where the object-space normal is shorter
                                than 1e-10 (:391-397) */
    float u;                 /* texture coordinate, see RT_SURFACE_HAS_UV */
    float shading_normal[3]; /* Ng, or the normal-mapped normal (:492-504) */
    float v;
    uint32_t triangle;       /* copied from the hit */
    uint32_t mesh;           /* copied from the hit */
    uint32_t submesh;        /* copied from the hit */
    uint32_t flags;          /* RT_SURFACE_* */
} rt_surface;

typedef struct rt_surface_material { /* 48 B */
    float base_color[3];     /* baseColor x the base-colour map */
    float opacity;           /* clamp(opacity x the opacity map, 0, 1) */
    float emission[3];       /* emission; an emission map replaces it (:453-456) */
    float ior;               /* max(refractionIndex, 1) */
    float roughness;         /* 1 without a roughness map, else the map's value, unclamped */
    float metallic;          /* 0 without a metallic map, else the map's value, unclamped */
    uint32_t texture_flags;  /* Material.textureFlags */
    uint32_t slot;           /* material slot: mesh * (largest submesh count of the scene) + submesh */
} rt_surface_material;
RT_STATIC_ASSERT(sizeof(rt_surface) == 64, "rt_surface is four 16-B words");
RT_STATIC_ASSERT(sizeof(rt_surface_material) == 48, "rt_surface_material is three 16-B words");

#define RT_SURFACE_HAS_UV       1u  /* the submesh has a bound map and (u, v) is the coordinate it is
                                        sampled at (after the v flip, :417); otherwise u = v = 0 */
#define RT_SURFACE_BACKFACE      2u  /* dot(direction, normal) > 0 */
#define RT_SURFACE_NORMAL_MAPPED 4u  /* the tangent basis was valid and the normal map was applied */
#define RT_SURFACE_TRANSMISSIVE  8u  /* the renderer's glass test: opacity < 0.999 || ior > 1.01 (:517) */

/* Semantics:
 *  - Hit data is used as given: t, u and v of the hit are not re-derived, so a caller may compact,
 *    reorder or edit hit records (with their rays).  `triangle` selects the geometry; mesh and
 *    submesh are copied through, the matrix and the material are looked up by the triangle's own
 *    instance and submesh.
 *  - A hit record whose `triangle` is RT_MISS, or at or above the scene's triangle count, is a
 *    miss and indexes nothing.  Its surface is position (0, 0, 0), t = INFINITY, zero normals and
 *    u, v, triangle = mesh = submesh = RT_MISS, flags 0; its material record is all zero.
 *  - materials == NULL skips that record and the base-colour, roughness, metallic and emission
 *    loads and samples.  The surface record is the same either way: the opacity (with its map)
 *    and the refraction index are read in both forms, RT_SURFACE_TRANSMISSIVE needs them.
 *  - Geometry seen, ordering against updates, rt_wait and rt_destroy: exactly as for
 *    rt_trace_closest above (the generation the next frame would read, after the update stream's
 *    work so far; updates first wait for pending resolves).  Frames rendered with resolves
 *    interleaved are bit-identical to frames rendered without.
 *  - The plain form runs on the context's stream, the _on form on `hip_stream` exactly as given.
 *    Back-to-back resolves and traces, also on different streams, need no host wait.
 *  - Errors: a NULL rays / hits / surfaces pointer with n > 0, or any pointer not 16-byte aligned:
 *    RT_ERR_INVALID_ARG.  Before a BVH build: RT_ERR_STATE.  n == 0: RT_OK, nothing is launched.
 *  - Statistics: a resolve is NOT folded into rt_query_stats; that struct (its last-query fields
 *    and its totals) describes traces only. */
rt_status rt_resolve_hits(rt_ctx* ctx, const rt_ray* rays, const rt_ray_hit* hits, uint32_t n, rt_surface* surfaces,
                          rt_surface_material* materials);
rt_status rt_resolve_hits_on(rt_ctx* ctx, const rt_ray* rays, const rt_ray_hit* hits, uint32_t n, rt_surface* surfaces,
                             rt_surface_material* materials, void* hip_stream);

/* ---- Shading queries: a resolved hit and its path state turned into the path's next rays -------
 * Everything raytracingKernel does between the material fetch and the next `intersect`
 * (Raytracing.metal:517-774): the glass branch (Fresnel choice, reflect / refract, transparency
 * passes), the light pick and the four light types, the GGX / legacy direct term with its shadow
 * ray, the cosine-hemisphere bounce, the throughput and the bounce / step bookkeeping, each drawing
 * from the renderer's own Halton dimension.  With the queries above the loop closes:
 *   trace -> resolve -> shade -> trace_any (shadow rays) + trace (next rays) -> resolve -> shade ...
 * and a caller runs the renderer's path tracer one bounce at a time: a frame re-assembled this way
 * (pixel = the sum of its samples' radiance in sample order / samples) equals rt_render_frame's
 * radiance of frame 0 bit for bit.
 *
 * One record per path, all DEVICE pointers, every record read and written as whole 16-B words. */
typedef struct rt_path {          /* 48 B, three 16-B words, 16-byte aligned */
    float    throughput[3];       /* the renderer's `color`; (1,1,1) at the camera */
    uint32_t sample;              /* the path's Halton index: random offset + frameIndex * stride + sample */
    float    radiance[3];         /* the renderer's `accum` */
    uint32_t flags;               /* RT_PATH_* */
    int32_t  bounce, step, transparency_passes;
    uint32_t reserved;            /* the record's tag: rt_shade_hits carries this word through unchanged;
                                     rt_camera_paths sets it, rt_retire_paths scatters by it (path
                                     queries, below); 0 where the caller has no use for it */
} rt_path;
#define RT_PATH_ALIVE  1u   /* in: shade this record; out: trace next_rays[i] again */
#define RT_PATH_SHADOW 2u   /* out: shadow_rays[i] / contrib[i] are live for this step */
RT_STATIC_ASSERT(sizeof(rt_path) == 48, "rt_path is three 16-B words");

typedef struct rt_shade_opts {    /* 32 B */
    int32_t shading_mode;         /* ShadingMode* of Uniforms */
    int32_t max_bounces;          /* 1 .. 12, as rt_render_frame accepts */
    int32_t light_count;          /* Uniforms.lightCount; 0 = every uploaded light */
    int32_t reserved[5];
} rt_shade_opts;
RT_STATIC_ASSERT(sizeof(rt_shade_opts) == 32, "rt_shade_opts is 32 B");

/* Semantics:
 *  - Inputs, per record: the ray that was traced (only its direction is read), its rt_surface and
 *    rt_surface_material from rt_resolve_hits (the material record is required here) and the path
 *    state.  `randoms` may be NULL.
 *  - Outputs: the path is updated in place (throughput, radiance with this hit's emission added,
 *    bounce / step / transparency_passes, flags).  next_rays[i] is the ray to trace next, tmax =
 *    INFINITY.  shadow_rays[i] is the light connection, tmax = lightDistance - 1e-3 (INFINITY for
 *    a sun light).  contrib[i] is (r, g, b, 0), four floats per record.
 *  - Bit-exactness: every float is the one the renderer's shading forms at that hit with the same
 *    path state: the PBR and the legacy mode, all four light types, glass, normal-mapped shading
 *    normals (already in the surface record).
 *  - Applying the shadow ray is the caller's, as the renderer does it: rt_trace_any on the flagged
 *    shadow rays, then radiance += contrib where not occluded.  The emission of this step is
 *    already in `radiance` (the renderer's order).
 *  - Record rules.  RT_PATH_SHADOW is an output: every call sets or clears it.
 *      ALIVE clear on input: the path is untouched but for SHADOW, which is cleared; the three
 *      output records are zero-filled with tmax = -1 on both rays.
 *      ALIVE set with bounce >= max_bounces, or with a miss surface (triangle == RT_MISS): ALIVE
 *      (and SHADOW) are cleared and nothing else changes (the renderer's `while` / `break`); the
 *      outputs are zero-filled as above.
 *      A step without a shadow ray: SHADOW is clear, shadow ray and contrib zero-filled, tmax = -1.
 *      A step that ends the path (throughput cut-off, last bounce): ALIVE is clear and the next
 *      ray is zero-filled with tmax = -1.
 *      Callers trace only flagged records; what the traversal does with a zero direction is not
 *      part of the interface.
 *  - randoms == NULL uses the renderer's Halton numbers at index paths[i].sample, dimensions
 *      light pick 2 + 6 step; area-light u, v 2 + 6 step + 1, + 2; glass choice 2 + 6 step + 5;
 *      hemisphere r0, r1 2 + 5 step + 3, 2 + 5 step + 4 (the reference's own 5-stride, :763-764).
 *    A dimension above the table's last (1023; the renderer's states stay below 944) reads the
 *    last.  Otherwise `randoms` holds n x 8 floats, two 16-B words per record:
 *    (light, area_u, area_v, glass_choice), (r0, r1, 0, 0), used in their place.
 *  - The light index is min((int)(x * count), count - 1) clamped to [0, count - 1], NaN -> 0: the
 *    renderer's index for every Halton value, and never one outside the lights for a caller's.
 *  - Not part of it: debug texture modes, the G-buffer, depth / motion, extra samples, the EMA.
 *  - The lights are the uploaded scene's (rt_scene_upload waits for pending queries first).  An
 *    effective light count of 0, or one above the uploaded count, is RT_ERR_INVALID_ARG.
 *  - Ordering against updates, streams, slots, rt_wait and rt_destroy: exactly as for
 *    rt_resolve_hits.  Not folded into rt_query_stats.  Frames rendered with shade queries
 *    interleaved are bit-identical to frames rendered without.  Needs the scene only (no BVH).
 *  - Errors: NULL opts, or any pointer but `randoms` NULL with n > 0: RT_ERR_INVALID_ARG.  Any
 *    pointer not 16-byte aligned, or an opts field out of range: RT_ERR_INVALID_ARG.  Before
 *    rt_scene_upload: RT_ERR_STATE.  n == 0: RT_OK, nothing is launched.
 *  - Aliasing: `paths` is updated in place; next_rays may alias rays (each record is read before
 *    it is written, by one thread).  No other two arrays may overlap. */
rt_status rt_shade_hits(rt_ctx* ctx, const rt_shade_opts* opts, const rt_ray* rays, const rt_surface* surfaces,
                        const rt_surface_material* materials, const float* randoms, uint32_t n, rt_path* paths,
                        rt_ray* next_rays, rt_ray* shadow_rays, float* contrib);
rt_status rt_shade_hits_on(rt_ctx* ctx, const rt_shade_opts* opts, const rt_ray* rays, const rt_surface* surfaces,
                           const rt_surface_material* materials, const float* randoms, uint32_t n, rt_path* paths,
                           rt_ray* next_rays, rt_ray* shadow_rays, float* contrib, void* hip_stream);

/* ---- Path queries: camera rays, stable compaction, connect, retire, average ----------------------
 * What a caller's loop does between the queries above, so that the whole integrator runs from
 * library calls (no framework glue, no host arithmetic):
 *   rt_camera_paths -> { rt_trace_closest -> rt_resolve_hits -> rt_shade_hits
 *                        -> rt_compact_paths(RT_PATH_SHADOW: shadow rays + index) -> rt_trace_any
 *                        -> rt_connect_paths -> rt_retire_paths
 *                        -> rt_compact_paths(RT_PATH_ALIVE: next rays + paths) } until count == 0
 *   -> rt_average_samples
 * equals rt_render_frame's radiance of frame 0 bit for bit, all four channels.  The host's only
 * part per round is reading the 4-byte count of each compaction (the `n` of the next launches),
 * and with the _indirect forms (device-count queries, below) not even that.
 *
 * All data pointers are DEVICE pointers.  Every call follows rt_resolve_hits' conventions: it
 * enqueues launches only (no host wait, no allocation in the steady state); the plain form runs
 * on the context's stream, the _on form on `hip_stream` exactly as given; each call takes one of
 * the ring of query slots, so back-to-back calls on different streams need no host wait;
 * rt_wait, rt_destroy and geometry updates wait for it; it is not folded into rt_query_stats;
 * n == 0 returns RT_OK with nothing launched (and nothing written); a NULL or misaligned pointer
 * is RT_ERR_INVALID_ARG on the host before any launch.  Record arrays are 16-byte aligned,
 * uint32_t arrays 4-byte aligned.  Frames rendered with these calls interleaved are bit-identical
 * to frames rendered without.  None of them needs a scene or a BVH. */
typedef struct rt_camera_opts {   /* 32 B */
    uint32_t first_pixel;         /* record i is pixel first_pixel + i, row-major */
    int32_t  sample;              /* sample number within the pixel, >= 0 */
    uint32_t tag_stride;          /* tag = pixel * tag_stride + tag_offset; >= 1 */
    uint32_t tag_offset;
    uint32_t reserved[4];
} rt_camera_opts;
RT_STATIC_ASSERT(sizeof(rt_camera_opts) == 32, "rt_camera_opts is 32 B");

typedef struct rt_compact_stream { /* 24 B */
    const void* src;
    void*       dst;
    uint32_t    words;            /* 16-B words per record, 1..4: 1 contrib; 2 rays, hits; 3 paths,
                                     materials; 4 surfaces */
    uint32_t    _pad;
} rt_compact_stream;
RT_STATIC_ASSERT(sizeof(rt_compact_stream) == 24, "rt_compact_stream is 24 B");

/* rt_camera_paths: the renderer's primary rays and path states.  Record i is pixel pix =
 * first_pixel + i (px = pix % width, py = pix / width of u->width x u->height).  Its Halton index
 * is the renderer's: random[pix] + frameIndex * (samplesPerPixel + maxExtra) + sample in uint32
 * arithmetic, maxExtra = enableMotionAdaptiveSampling ? max(motionSamplingMaxExtraSamples, 0) : 0.
 * rays[i] is the renderer's primary ray of that index (origin word 3 = 0, tmax = INFINITY);
 * paths[i] is throughput 1, `sample` = the Halton index, radiance 0, flags RT_PATH_ALIVE, bounce =
 * step = transparency_passes = 0, tag (`reserved`) = pix * tag_stride + tag_offset.
 * random_offsets: a device array of width * height words, or NULL = the context's own from
 * rt_resize (RT_ERR_STATE without one, or when its size is not u->width x u->height).
 * RT_ERR_INVALID_ARG: first_pixel + n > width * height, a non-positive size, sample < 0,
 * tag_stride == 0.  Reads no scene and no BVH. */
rt_status rt_camera_paths(rt_ctx* ctx, const Uniforms* u, const rt_camera_opts* opts, const uint32_t* random_offsets,
                          uint32_t n, rt_ray* rays, rt_path* paths);
rt_status rt_camera_paths_on(rt_ctx* ctx, const Uniforms* u, const rt_camera_opts* opts, const uint32_t* random_offsets,
                             uint32_t n, rt_ray* rays, rt_path* paths, void* hip_stream);

/* rt_compact_paths: stable stream compaction by path flags.  The selected set is every i < n with
 * (paths[i].flags & mask) != 0, m of them.  For the j-th selected record in ascending i:
 * dst_k[j] = src_k[i] for each of the stream_count (0..4) streams, as whole 16-B words;
 * index[j] = i unless index is NULL; *count = m.  Nothing is written at or beyond m.  The result
 * is what a[(flags & mask) != 0] gives in numpy: stable, deterministic, identical from call to
 * call.  Three launches: per-tile counts and a selection bitmask, a one-block scan of the tile
 * counts, per-tile rank and copy; no block waits for another.  Temporary storage (132 B per 1024
 * records) belongs to the call's query slot, grows on demand and is counted in
 * rt_stats.device_bytes.
 * `paths` may itself be a src.  NOT in place: no dst (nor index, nor count) may overlap any src,
 * any other dst or paths; the call can only check that the base pointers differ.
 * RT_ERR_INVALID_ARG: mask == 0, stream_count > 4, words outside 1..4, equal base pointers. */
rt_status rt_compact_paths(rt_ctx* ctx, const rt_path* paths, uint32_t n, uint32_t mask, const rt_compact_stream* streams,
                           uint32_t stream_count, uint32_t* index, uint32_t* count);
rt_status rt_compact_paths_on(rt_ctx* ctx, const rt_path* paths, uint32_t n, uint32_t mask,
                              const rt_compact_stream* streams, uint32_t stream_count, uint32_t* index, uint32_t* count,
                              void* hip_stream);

/* rt_connect_paths: applies traced shadow rays.  For j < m with occluded[j] == 0 and
 * i = index ? index[j] : j: paths[i].radiance += contrib[i].rgb (contrib: four floats per record,
 * as rt_shade_hits writes them; three fp32 adds, the renderer's accum = accum + contrib); nothing
 * else in the record changes.  An i >= n is skipped and never dereferenced.  The index entries
 * must be distinct (rt_compact_paths' are): otherwise two threads update one record. */
rt_status rt_connect_paths(rt_ctx* ctx, rt_path* paths, uint32_t n, const float* contrib, const uint32_t* index,
                           const uint32_t* occluded, uint32_t m);
rt_status rt_connect_paths_on(rt_ctx* ctx, rt_path* paths, uint32_t n, const float* contrib, const uint32_t* index,
                              const uint32_t* occluded, uint32_t m, void* hip_stream);

/* rt_retire_paths: for every record with RT_PATH_ALIVE clear and tag < tags,
 * samples[tag] = (radiance.r, radiance.g, radiance.b, 1.0f), one 16-B store.  A pure scatter: with
 * distinct tags the result does not depend on order.  A tag at or above `tags` is skipped. */
rt_status rt_retire_paths(rt_ctx* ctx, const rt_path* paths, uint32_t n, float* samples, uint32_t tags);
rt_status rt_retire_paths_on(rt_ctx* ctx, const rt_path* paths, uint32_t n, float* samples, uint32_t tags,
                             void* hip_stream);

/* rt_average_samples: rgba[p].rgb = (((s[p*spp] + s[p*spp+1]) + ...) + s[p*spp+spp-1]) / (float)spp
 * in fp32, in sample order (the renderer's resolve of frame 0); alpha = 1.0f as the renderer stores
 * it.  spp is 1..64.  No EMA, no motion, no G-buffer. */
rt_status rt_average_samples(rt_ctx* ctx, const float* samples, uint32_t pixels, uint32_t spp, float* rgba);
rt_status rt_average_samples_on(rt_ctx* ctx, const float* samples, uint32_t pixels, uint32_t spp, float* rgba,
                                void* hip_stream);

/* ---- Device-count queries: the record count read on the device ------------------------------------
 * The indirect-dispatch form of the seven queries whose `n` a compaction produces.  The count
 * stays in device memory: rt_compact_paths_indirect writes it, the next queries read it, and the
 * host never waits for it.  Each signature is the direct form's with `uint32_t n` replaced by
 * `const rt_device_count* cnt` (rt_connect_paths_indirect: its `m`; its `n` stays a host bound).
 * Both entry points of a query have one: X_indirect runs on the context's stream as X does,
 * X_on_indirect on `hip_stream` as X_on does (the suffix names the form of that entry point).
 * The struct itself is host memory, read before the call returns.  rt_camera_paths and
 * rt_average_samples have no such form: the host knows their sizes.
 *   rt_compact_paths_indirect(.., &in, .., &out_word) -> rt_trace_closest_indirect(.., {&out_word, max}, ..)
 *   -> rt_resolve_hits_indirect(.., {&out_word, max}, ..) -> ...   with no host wait anywhere. */
typedef struct rt_device_count {   /* 16 B */
    const uint32_t* count;         /* DEVICE pointer, 4-byte aligned: the number of records, read on
                                      the device when the launch runs */
    uint32_t        max;           /* host bound: the arrays hold this many records */
    uint32_t        _pad;
} rt_device_count;
RT_STATIC_ASSERT(sizeof(rt_device_count) == 16, "rt_device_count is 16 B");

/* Semantics:
 *  - Effective count: min(*cnt->count, cnt->max), read once per launch on the device, ordered on
 *    the stream the query runs on: a `count` written by an earlier rt_compact_paths* on the same
 *    stream is the one seen, with no host wait between.  The library never reads `count` on the
 *    host.
 *  - Records at or beyond the effective count are neither read nor written.  A *count above max
 *    clamps to max; nothing past max is addressed.
 *  - The host uses `max` wherever the direct form uses `n`: the pointer checks, the grid size, the
 *    compaction's temporary storage, the early return.
 *  - max == 0: RT_OK, nothing is launched and nothing is written (`count` may then be NULL).
 *  - An effective count of 0 with max > 0 is a normal launch: it writes no record;
 *    rt_compact_paths_indirect still writes *count_out = 0; a trace still counts as a query in
 *    rt_query_stats, with rays == 0.
 *  - rt_compact_paths_indirect chains: *count_out is always written when max > 0, so it can be the
 *    next call's cnt->count.  count_out == cnt->count is RT_ERR_INVALID_ARG (the copy launch
 *    reads the input count after the scan launch wrote the output).
 *  - Statistics: for the indirect traces rt_query_stats.rays, hits, node_visits and tri_tests are
 *    the device-counted figures of the effective count; grid_blocks is what `max` gave.
 *  - Geometry generation, ordering against updates, query slots, rt_wait, rt_destroy, aliasing
 *    and the guarantee that frames rendered with queries interleaved are bit-identical: exactly
 *    as for the direct forms.  The results of the first `effective count` records are the direct
 *    form's with n = that count, bit for bit.
 *  - Errors: cnt == NULL, cnt->count == NULL with max > 0, or a count pointer not 4-byte aligned:
 *    RT_ERR_INVALID_ARG before any launch; then the direct form's errors with n = max.
 *  - Lifetime: the caller keeps `count` alive, and does not write it, until the query has
 *    finished. */
rt_status rt_trace_closest_indirect(rt_ctx* ctx, const rt_ray* rays, const rt_device_count* cnt, rt_ray_hit* hits);
rt_status rt_trace_closest_on_indirect(rt_ctx* ctx, const rt_ray* rays, const rt_device_count* cnt, rt_ray_hit* hits,
                                       void* hip_stream);
rt_status rt_trace_any_indirect(rt_ctx* ctx, const rt_ray* rays, const rt_device_count* cnt, uint32_t* occluded);
rt_status rt_trace_any_on_indirect(rt_ctx* ctx, const rt_ray* rays, const rt_device_count* cnt, uint32_t* occluded,
                                   void* hip_stream);
rt_status rt_resolve_hits_indirect(rt_ctx* ctx, const rt_ray* rays, const rt_ray_hit* hits, const rt_device_count* cnt,
                                   rt_surface* surfaces, rt_surface_material* materials);
rt_status rt_resolve_hits_on_indirect(rt_ctx* ctx, const rt_ray* rays, const rt_ray_hit* hits, const rt_device_count* cnt,
                                      rt_surface* surfaces, rt_surface_material* materials, void* hip_stream);
rt_status rt_shade_hits_indirect(rt_ctx* ctx, const rt_shade_opts* opts, const rt_ray* rays, const rt_surface* surfaces,
                                 const rt_surface_material* materials, const float* randoms, const rt_device_count* cnt,
                                 rt_path* paths, rt_ray* next_rays, rt_ray* shadow_rays, float* contrib);
rt_status rt_shade_hits_on_indirect(rt_ctx* ctx, const rt_shade_opts* opts, const rt_ray* rays, const rt_surface* surfaces,
                                    const rt_surface_material* materials, const float* randoms, const rt_device_count* cnt,
                                    rt_path* paths, rt_ray* next_rays, rt_ray* shadow_rays, float* contrib,
                                    void* hip_stream);
rt_status rt_compact_paths_indirect(rt_ctx* ctx, const rt_path* paths, const rt_device_count* cnt, uint32_t mask,
                                    const rt_compact_stream* streams, uint32_t stream_count, uint32_t* index,
                                    uint32_t* count);
rt_status rt_compact_paths_on_indirect(rt_ctx* ctx, const rt_path* paths, const rt_device_count* cnt, uint32_t mask,
                                       const rt_compact_stream* streams, uint32_t stream_count, uint32_t* index,
                                       uint32_t* count, void* hip_stream);
rt_status rt_connect_paths_indirect(rt_ctx* ctx, rt_path* paths, uint32_t n, const float* contrib, const uint32_t* index,
                                    const uint32_t* occluded, const rt_device_count* cnt);
rt_status rt_connect_paths_on_indirect(rt_ctx* ctx, rt_path* paths, uint32_t n, const float* contrib,
                                       const uint32_t* index, const uint32_t* occluded, const rt_device_count* cnt,
                                       void* hip_stream);
rt_status rt_retire_paths_indirect(rt_ctx* ctx, const rt_path* paths, const rt_device_count* cnt, float* samples,
                                   uint32_t tags);
rt_status rt_retire_paths_on_indirect(rt_ctx* ctx, const rt_path* paths, const rt_device_count* cnt, float* samples,
                                      uint32_t tags, void* hip_stream);

/* Library build identification (kernel code object arch etc). */
const char* rt_version(void);

/* Test hook (host only, no device): build the library's BVH for `scene` and trace `n` rays
 * (6 floats each: origin, direction) with the traversal code the kernels use, compiled for the
 * host.  any = 0: closest hit, 1: any hit; tmax per ray or NULL (= infinity).  Outputs per ray:
 * t (inf on miss), original triangle id (0xffffffff on miss), barycentrics u/v, BVH nodes
 * fetched and triangles tested (u, v, nodes, tris may be NULL). */
rt_status rt_debug_trace_host(const rt_scene_desc* scene, const float* rays, const float* tmax, uint32_t n,
                              int32_t any, float* t, uint32_t* id, float* u, float* v, uint32_t* nodes,
                              uint32_t* tris);

/* Test hook (host only, no device): rt_resolve_hits over a scene description, by the code the
 * kernel runs, compiled for the host.  All pointers are HOST pointers here; `materials` may be
 * NULL.  The scene is checked as rt_scene_upload checks it.  Any material, normal maps and
 * base-colour maps included. */
rt_status rt_debug_resolve_host(const rt_scene_desc* scene, const rt_ray* rays, const rt_ray_hit* hits, uint32_t n,
                                rt_surface* surfaces, rt_surface_material* materials);

/* Test hook (host only, no device): rt_shade_hits over host arrays and the given lights, by the
 * code the kernel runs, compiled for the host.  All pointers are HOST pointers; the same checks
 * (light_count here is the number of lights given; opts->light_count 0 = all of them). */
rt_status rt_debug_shade_host(const Light* lights, uint32_t light_count, const rt_shade_opts* opts, const rt_ray* rays,
                              const rt_surface* surfaces, const rt_surface_material* materials, const float* randoms,
                              uint32_t n, rt_path* paths, rt_ray* next_rays, rt_ray* shadow_rays, float* contrib);

/* Test hook (host only, no device): rt_camera_paths over host arrays, by the code the kernel runs,
 * compiled for the host.  All pointers are HOST pointers; random_offsets is required (width *
 * height words); the same checks. */
rt_status rt_debug_camera_paths_host(const Uniforms* u, const rt_camera_opts* opts, const uint32_t* random_offsets,
                                     uint32_t n, rt_ray* rays, rt_path* paths);

/* Test hook (host only, no device): rt_compact_paths over host arrays, a sequential loop; the same
 * checks. */
rt_status rt_debug_compact_paths_host(const rt_path* paths, uint32_t n, uint32_t mask, const rt_compact_stream* streams,
                                      uint32_t stream_count, uint32_t* index, uint32_t* count);

/* Test hooks (host only, no device): what every frame after the first adds to the path queries'
 * loop, as per-record code compiled for the host over HOST pointers (no device query of theirs
 * exists yet).  The arithmetic is the frame kernels' own functions: depth and motion of sample 0's
 * bounce-0 hits (Raytracing.metal:342-389), the motion-adaptive extra samples (:777-789), the
 * resolve with the accumulation against the history (:792-819).  Frames assembled from these hooks
 * and the ones above equal the oracle's bit for bit in radiance, depth and motion.
 *
 * rt_debug_primary_outputs_host: called before the shade hook of the same round, so `paths` holds
 * the state at the hit.  A record is used when RT_PATH_ALIVE is set, bounce == 0, its tag is
 * selected by `opts` and the hit's `triangle` is below the scene's triangle count; depth[pixel] and
 * motion[pixel] (two fp32 per pixel, as rt_read_aux returns them) then get what the renderer
 * computes from the hit's triangle, u and v, u->camera and u->previousCamera.  Every other record
 * writes nothing.  Once per round, in order, gives the renderer's "last bounce-0 hit of sample 0
 * wins" for glass paths.  The scene is a description (checked as rt_scene_upload checks it) with
 * the previous instance transforms, one per mesh (NULL = the current ones); its previous positions
 * are the current positions.  A pixel the renderer's sample 0 never hits keeps depth 1.0e8f and
 * motion (0, 0): the caller's fill.
 *
 * rt_debug_extra_paths_host: maxExtra is rt_camera_paths' definition.  For pixel pix =
 * opts->first_pixel + i: extra[i] = the renderer's extra-sample count from motion[pix] and
 * motion_prev[pix] (NULL: zeros).  For j < maxExtra, record i * maxExtra + j of rays / paths is the
 * rt_camera_paths record of sample opts->sample + j (the caller passes samplesPerPixel) with tag
 * pix * tag_stride + tag_offset + j when j < extra[i], otherwise zero-filled with flags 0 and
 * tmax = -1.  With maxExtra == 0 only `extra` is written; rays and paths may be NULL.
 * random_offsets is required; otherwise rt_camera_paths' checks.
 *
 * rt_debug_resolve_samples_host: with spp = u->samplesPerPixel and e = extra ? extra[p] : 0 (an e
 * above sample_stride - spp counts as that), total = the first spp + e samples of pixel p summed
 * in sample order / their number; when u->frameIndex > 0, mixed with history[p] by the renderer's
 * motion-adaptive history weight (a NULL motion target reads as zeros).  Alpha 1.0f.  At frame 0
 * with extra == NULL and sample_stride == spp: rt_average_samples' arithmetic.
 * RT_ERR_INVALID_ARG: history == NULL with frameIndex > 0, spp outside 1 .. 64,
 * spp + maxExtra > sample_stride, rgba == history or samples.
 * Alignment: record arrays, samples, history, rgba 16-byte; motion targets 8-byte; others 4-byte. */
typedef struct rt_target_opts {   /* 32 B */
    uint32_t tag_stride;          /* >= 1: pixel = tag / tag_stride */
    uint32_t tag_offset;          /* a record is selected when tag % tag_stride == tag_offset (sample 0's) */
    uint32_t pixels;              /* depth / motion hold this many pixels; a pixel at or above it is skipped */
    uint32_t reserved[5];
} rt_target_opts;
RT_STATIC_ASSERT(sizeof(rt_target_opts) == 32, "rt_target_opts is 32 B");
rt_status rt_debug_primary_outputs_host(const rt_scene_desc* scene, const rt_packed_float4x3* prev_transforms,
                                        const Uniforms* u, const rt_target_opts* opts, const rt_ray_hit* hits,
                                        const rt_path* paths, uint32_t n, float* depth, float* motion);
rt_status rt_debug_extra_paths_host(const Uniforms* u, const rt_camera_opts* opts, const uint32_t* random_offsets,
                                    const float* motion, const float* motion_prev, uint32_t n, rt_ray* rays, rt_path* paths,
                                    uint32_t* extra);
rt_status rt_debug_resolve_samples_host(const Uniforms* u, const float* samples, uint32_t sample_stride,
                                        const uint32_t* extra, const float* motion, const float* motion_prev,
                                        const float* history, uint32_t pixels, float* rgba);

#ifdef __cplusplus
}
#endif
#endif /* RT_API_H */
