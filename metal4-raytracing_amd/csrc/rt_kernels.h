// rt_kernels.h — FrameParams, the statistics flush and the launch entry points of the megakernel, the
// on-device BVH build and the utility kernels (device code lives in *.hip; the wavefront pipeline: rt_wavefront.h).
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "rt_device.h"

namespace rt {

constexpr int kHaltonLds = 64;   // first Halton dimensions staged in LDS per block

// kCntNodes: every node test.  Slot 9 is unused (formerly LDS-served node tests).
// kCntTrace*: the share of the visits made by wf_trace launches.
// kCntRootRetired: closest-hit rays their producer retired on root mask 0 (also in kCntClosest).
// Past kCntSlots, the shadow rays a shading step resolved without a traversal (flushed by the kernels
// that shade: block_flush_counters<true>; each also in kCntShadow): kCntDarkShadow with a
// contribution of ±0 (shadow_is_dark), kCntRootUnoccluded proven unoccluded by root mask 0;
// kCntShadeSkipped: those of either class that wf_shade resolved, which a connect launch would
// have traced.
enum CounterSlot {
    kCntClosest = 0, kCntShadow = 1, kCntNodes = 2, kCntTris = 3, kCntPaths = 4, kCntOverflow = 5,
    kCntTraceNodes = 6, kCntTraceTris = 7, kCntRootRetired = 8, kCntSlots = 10,
    kCntDarkShadow = 10, kCntRootUnoccluded = 11, kCntShadeSkipped = 12, kCntSlotsAll = 13
};

struct FrameParams {
    Uniforms U;
    const uint32_t* random;
    const float4* accum_in;    // history (TextureIndexAccumulation, read)
    float4* accum_out;         // new accumulation (TextureIndexPreviousAccumulation, write)
    float* depth;
    float2* motion;            // read (previous frame) + write, in place
    const float2* motion_prev; // wavefront: the previous frame's motion target (it writes a new one)
    float4* gbuffer;           // 4 planes or null
    uint4* prim_hit;           // wavefront: sample 0's last bounce-0 hit per pixel (wf_motion input)
    unsigned long long* counters;
    int tile_size, rank, nranks, tiles_x;
};

__device__ __forceinline__ unsigned long long wave_sum(uint32_t v) {
    unsigned long long s = v;
    #pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    return s;
}

// Statistics counters: every (slot, replica) word sits on a 128-B line of its own and a block adds
// to replica blockIdx % 8 once per slot, so no line sees more than ~1/8 of the blocks' atomics
// (device-scope atomics on one line serialise at ~88/us).  The host sums the replicas.
constexpr int kCntReplicas = 8;
constexpr int kCntLineU64 = 16;
constexpr int kCounterWords = kCntSlotsAll * kCntReplicas * kCntLineU64;
__host__ __device__ constexpr uint32_t cnt_word(int slot, int rep) {
    return ((uint32_t)slot * kCntReplicas + (uint32_t)rep) * kCntLineU64;
}

// Block-wide flush of the per-thread statistics; every thread of the block must call it.
// nodes: global node fetches, lds_nodes: node tests served from LDS (both count as node visits).
// trace_kernel: the node / triangle visits are also added to the kCntTrace* slots.
// SKIPS (the kernels that shade): also the shadow rays their steps resolved without a traversal,
// dark and root_unoccluded by class, shade_skipped those of both that wf_shade resolved.
template <bool SKIPS = false>
__device__ __forceinline__ void block_flush_counters(unsigned long long* counters, uint32_t closest, uint32_t shadow,
                                                     uint32_t nodes, uint32_t tris, uint32_t paths, bool overflow,
                                                     bool trace_kernel = false, uint32_t lds_nodes = 0,
                                                     uint32_t root_retired = 0, uint32_t dark = 0,
                                                     uint32_t root_unoccluded = 0, uint32_t shade_skipped = 0) {
    constexpr int kN = SKIPS ? kCntSlotsAll : kCntSlots;
    __shared__ unsigned long long red[kBlock / 64][kN];
    const unsigned long long l = wave_sum(lds_nodes), n = wave_sum(nodes) + l, t = wave_sum(tris);
    const unsigned long long v[kCntSlotsAll] = {wave_sum(closest), wave_sum(shadow), n, t, wave_sum(paths),
                                                __ballot(overflow) != 0ull ? 1ull : 0ull,
                                                trace_kernel ? n : 0ull, trace_kernel ? t : 0ull, wave_sum(root_retired),
                                                trace_kernel ? l : 0ull,
                                                SKIPS ? wave_sum(dark) : 0ull, SKIPS ? wave_sum(root_unoccluded) : 0ull,
                                                SKIPS ? wave_sum(shade_skipped) : 0ull};
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        #pragma unroll
        for (int k = 0; k < kN; ++k) red[wave][k] = v[k];
    }
    __syncthreads();
    if (threadIdx.x < kN) {
        unsigned long long s = 0;
        #pragma unroll
        for (int w = 0; w < kBlock / 64; ++w) s += red[w][threadIdx.x];
        if (s) atomicAdd(&counters[cnt_word(threadIdx.x, blockIdx.x & (kCntReplicas - 1))], s);
    }
}

void launch_megakernel(const DevScene& S, const FrameParams& P, int nblocks, bool count, hipStream_t stream);

// Packed-tile layout of the multi-GPU gather: element i of a rank's packed buffer is pixel
// (i % T, (i / T) % T) of its (i / T^2)-th own tile; own tile k is tile id rank + k * nranks.
__host__ __device__ __forceinline__ void tile_pixel(size_t i, int tile, int rank, int nranks, int tiles_x, int& x,
                                                    int& y) {
    const size_t per = (size_t)tile * tile;
    const int k = (int)(i / per), r = (int)(i % per);
    const int tid = rank + k * nranks;
    x = (tid % tiles_x) * tile + r % tile;
    y = (tid / tiles_x) * tile + r / tile;
}

// On-device BVH build (rt_lbvh.hip): LBVH over Morton codes collapsed into the compressed 8-wide
// layout of rt_bvh.h.  Inputs are the uploaded scene streams; outputs are caller-allocated device
// arrays sized for n triangles (nodes8 / node_box / levels: n entries, tri_order n, tri_bin n).
struct LbvhInput {
    const float4* pos;
    const uint4* tri_info;
    const float* inst;
    uint32_t n;
    int ploc = 1;          // BVH2 topology: 1 = PLOC clustering, 0 = LBVH radix tree (8-wide: SAH-DP collapse)
    float c_node = 1.0f;   // DP costs (as the host builder's)
    float c_prim = 0.5f;
};
struct LbvhOutput {
    Bvh8Node* nodes8;
    float* node_box;        // 6 floats per node (padded lo, hi)
    uint32_t* tri_order;    // 8-wide triangle slot -> original triangle id
    uint16_t* tri_bin;      // hit-sort bin per original triangle
    uint32_t* levels;       // refit level list (the identity: nodes are allocated level by level)
    uint32_t* h_scratch;    // 1 pinned host word
};
struct LbvhResult {
    std::vector<uint32_t> level_off;   // level k = nodes [level_off[k], level_off[k + 1])
    uint32_t num_nodes = 0;
    int max_depth = 0;
    float pad = 0.0f;
};
size_t lbvh_scratch_bytes(uint32_t n);
bool lbvh_build(const LbvhInput& in, const LbvhOutput& out, void* scratch, hipStream_t s, LbvhResult* res,
                const char** err);

// Device ray queries (rt_query.hip): one persistent launch of rq_trace over a flat array of n
// caller rays (two 16-B words each: origin, direction + tmax).  `state` is the launch's own device
// block, zeroed before it: the statistics counters (kCounterWords, block_flush_counters' layout:
// kCntClosest / kCntShadow rays, kCntPaths rays that hit / are occluded, nodes, triangles,
// overflow), then kRqChunkCounters chunk counters, one per 128-B line.
constexpr int kRqChunk = 64;          // rays per chunk grab
constexpr int kRqChunkCounters = 8;   // one per XCD (blockIdx % 8)
constexpr size_t kRqStateBytes = sizeof(unsigned long long) * kCounterWords + 128 * kRqChunkCounters;

// The record count of a query launch.  Every rq_* parameter block carries the host's count and a
// device word `count` that is null for the direct forms.  With a word (the _indirect forms of
// include/rt_api.h) the host's count is only a bound: the launch runs over min(*count, bound),
// read once at kernel entry and kept in a scalar register, so every loop bound stays wave-uniform.
// The word was written by an earlier launch on the stream (the kernel boundary orders it).
__device__ __forceinline__ uint32_t launch_count(const uint32_t* count, uint32_t bound) {
    if (!count) return bound;
    const uint32_t v = *count;
    return __builtin_amdgcn_readfirstlane(v < bound ? v : bound);
}

struct RqParams {
    const float4* rays;
    float4* hits;               // closest hit: two 16-B words per ray (rt_ray_hit)
    uint32_t* occluded;         // any hit: one word per ray
    const uint32_t* sub_first;  // first scene-wide triangle id of submesh [mesh * max_submeshes + submesh]
    unsigned long long* state;
    const uint32_t* count;      // or null (launch_count)
    uint32_t n;
    int refill_min;
};
// resident blocks (CUs x blocks per CU) of the query kernels
unsigned query_resident_blocks();
void launch_query(const DevScene& S, const RqParams& Q, bool any, bool count, unsigned blocks, hipStream_t stream);

// Surface queries (rq_resolve, rt_query.hip): one thread per record turns a ray and its hit into
// an rt_surface (four 16-B words) and, unless `materials` is null, an rt_surface_material (three),
// by surface_eval (rt_surface.h).  S carries the shading streams (tri_nrm, inst, materials and,
// for a textured scene, the texture tables); the tree is not read.
struct RsParams {
    const float4* rays;     // two words per record (rt_ray)
    const float4* hits;     // two words per record (rt_ray_hit)
    float4* surfaces;
    float4* materials;      // or null
    const uint32_t* count;  // or null (launch_count)
    uint32_t n;
};
unsigned resolve_resident_blocks();
void launch_resolve(const DevScene& S, const RsParams& P, unsigned blocks, hipStream_t stream);

// Shading queries (rq_shade, rt_query.hip): one thread per record turns the traced ray's direction,
// its surface and material records and the path state into the updated path, the next ray, the
// shadow ray and its contribution, by scatter_eval (rt_scatter.h).  Lights and the Halton table
// are the context's; nothing else of the scene is read.
struct ShParams {
    const float4* rays;        // two words per record (rt_ray); the second is read
    const float4* surfaces;    // four words per record (rt_surface)
    const float4* materials;   // three (rt_surface_material)
    const float4* randoms;     // two, or null: the renderer's Halton numbers
    float4* paths;             // three (rt_path), in place
    float4* next_rays;         // two; may alias rays
    float4* shadow_rays;       // two
    float4* contrib;           // one
    const Light* lights;
    const HaltonDim* halton;
    const uint32_t* count;     // or null (launch_count)
    uint32_t n;
    int shading_mode, max_bounces, light_count;
};
unsigned shade_resident_blocks();
void launch_shade(const ShParams& P, unsigned blocks, hipStream_t stream);

// Path queries (rq_camera, rq_connect, rq_retire, rq_average and the three rq_compact_* launches,
// rt_query.hip; per-record code and tile geometry: rt_paths.h).  One thread per record but for the
// compaction, all records as 16-B words.
struct CamParams {
    Uniforms U;
    const uint32_t* random;    // width * height offsets
    const HaltonDim* halton;   // the table; entry 1 is read
    float4* rays;              // two words per record
    float4* paths;             // three
    uint32_t n, first_pixel, tag_stride, tag_offset;
    int sample;
};
struct ConnectParams {
    float4* paths;
    const float4* contrib;
    const uint32_t* index;     // or null: j itself
    const uint32_t* occluded;
    const uint32_t* count;     // or null (launch_count): bounds m, never n
    uint32_t n, m;
};
struct RetireParams {
    const float4* paths;
    float4* samples;
    const uint32_t* count;     // or null (launch_count)
    uint32_t n, tags;
};
struct AverageParams {
    const float4* samples;
    float4* rgba;
    uint32_t pixels, spp;
};
struct CompactParams {
    const float4* paths;
    const float4* src[4];
    float4* dst[4];
    uint32_t words[4];
    uint32_t* index;                // or null
    uint32_t* count;
    unsigned long long* bits;       // kCompactSegs selection words per tile
    uint32_t* tile_count;           // per tile: selected count, after the scan its offset
    const uint32_t* n_count;        // or null (launch_count): the input count; never equal to `count`
    uint32_t n, mask, streams, tiles;   // tiles = compact_tiles(n): what bits / tile_count are sized and laid out for
};
unsigned path_resident_blocks();
void launch_camera(const CamParams& P, unsigned blocks, hipStream_t stream);
void launch_connect(const ConnectParams& P, unsigned blocks, hipStream_t stream);
void launch_retire(const RetireParams& P, unsigned blocks, hipStream_t stream);
void launch_average(const AverageParams& P, unsigned blocks, hipStream_t stream);
// the three launches of a compaction; tile_blocks: the grid of the count and the copy launch
void launch_compact(const CompactParams& P, unsigned tile_blocks, hipStream_t stream);

// Utility kernels (rt_util.hip)
// G-buffer-guided denoise for RT_SCALER_DENOISED (rt_present.hip); returns tmp0 or tmp1, whichever
// holds the result (passes = 0 returns the demodulated radiance unremodulated: callers pass >= 1)
const float4* launch_denoise(const float4* accum, const float* depth, const float4* gbuf, float4* tmp0, float4* tmp1,
                             float4* guide, float4* alb, int w, int h, int passes, hipStream_t stream);
void launch_present(const float4* accum, const float* depth, const float2* motion, const float4* hist_in,
                    const float* hdepth_in, float4* hist_out, float* hdepth_out, uchar4* out, const float* thr, int w,
                    int h, int ow, int oh, int scaler, int srgb, int use_hist, hipStream_t stream);
void launch_pack_tiles(const float4* src, float4* dst, int width, int height, int tile, int rank, int nranks,
                       int tiles_x, int own, hipStream_t s);
void launch_unpack_tiles(const float4* src, float4* dst, int width, int height, int tile, int rank, int nranks,
                         int tiles_x, int own, hipStream_t s);
void launch_to_half(const float4* src, ushort4* dst, size_t n, hipStream_t s);
// sum of the node boxes' areas (node_box: 6 floats per node), one float out
void launch_bvh_cost(const float* node_box, uint32_t nn, float* out, hipStream_t s);
void launch_skin(const float4* rest_pos, const float4* rest_nrm, const ushort4* jidx, const float4* jw,
                 const float* joints, float4* out_pos, float4* out_nrm, uint32_t n, hipStream_t s);
// flatten also reduces max |world coordinate| into *maxabs_bits (float bits; zero it first)
void launch_flatten(const uint4* tri_info, const uint32_t* slot_to_tri, const float4* pos, const float* inst,
                    float* tris, uint32_t n, unsigned* maxabs_bits, hipStream_t s);
// per-triangle shading records of triangles [t0, t0 + n) (DevScene::tri_nrm) from tri_info and the
// vertex normals; rebuilt whenever normals change (scene upload, skinning)
void launch_tri_nrm(const uint4* tri_info, const float4* nrm, float4* tri_nrm, uint32_t t0, uint32_t n, hipStream_t s);
// the fp32 bounds of the root's eight child slots (rt_device.h RootBoxes) from the tree as it stands
void launch_root_boxes(const Bvh8Node* nodes, const float* node_box, const float* tris, RootBoxes* out, hipStream_t s);
// pad = max(pad_min, 4e-6 * max |coordinate|) as the builder pads (rt_bvh.cpp)
void launch_refit8_level(Bvh8Node* nodes, float* node_box, const float* tris, const uint32_t* level_nodes,
                         uint32_t count, float pad_min, const unsigned* maxabs_bits, hipStream_t s);

}  // namespace rt
