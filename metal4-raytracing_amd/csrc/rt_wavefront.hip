// rt_wavefront.hip — wavefront path tracer for gfx950.
//
// The per-pixel loop of raytracingKernel (Raytracing.metal:269-790) is split into stages over
// SoA path state and compacted queues, so every wave64 works on live paths only:
//   generate  one thread per (own pixel, sample): primary ray (:270-292) -> ray queue, with the
//             ray's root word (the BVH root's 8-wide test on the exact boxes of its children,
//             root_word_tight); a ray that misses them all is a proven miss and is not enqueued
//   extend    closest-hit traversal of the ray queue (:314-322)          -> hit records; a ray
//             with a root word starts at the root's result (trav_start_root), one step later
//   shade     shade_step per hit (:324-774): updates path state, appends the continuation
//             ray to the next queue and the NEE shadow ray to the shadow queue, each with its
//             root word (a continuation ray with root mask 0 is not appended: its path ends as
//             after a miss; a shadow ray with root mask 0 is not appended either: it is proven
//             unoccluded and shade adds its contribution itself; nor is a dark one, whose
//             contribution of ±0 cannot change accum, shade_step); a block first compacts the hits
//             of its queue entries, so a missed ray takes no lane
//   connect   any-hit traversal of the shadow queue (:716-743); unoccluded -> accum += contrib;
//             starts from the shadow ray's root word as extend does
//   finish    once fewer than kTailRays paths are alive, one launch runs every remaining path
//             to completion (trace -> shade -> shadow per thread): the long glass-path tail
//             costs the longest remaining path instead of one launch per bounce
//   [extra]   motion-adaptive extra samples (:779-789) as a second generate/iterate pass (no root
//             words: its entries carry 0 and extend tests the root itself)
//   resolve   per pixel: sum samples in sample order, average, temporal EMA (:777, :792-819)
//
// Results are bit-identical to the megakernel: per-path arithmetic is the same shade_step,
// the accumulation order per path is the reference's (emission of step s, then its shadow
// contribution -- added by connect, or by shade for a ray it proved unoccluded -- then step s+1),
// and samples are summed per pixel in sample order.
//
// This file holds the kernels only: the sharded queues and the index maths are rt_wf_queue.h, the
// stepwise traversal rt_trav.h, the counter words rt_wf_counters.h; rt_wavefront_host.cpp launches
// the kernels, through wf_kernels() below.
#include "rt_shade.h"
#include "rt_trav.h"
#include "rt_wavefront.h"
#include "rt_wf_queue.h"

#include <array>
#include <utility>

namespace rt {

namespace {

constexpr uint32_t kNoKey = 0xffffffffu;       // sort key of a miss (dropped by the sort)

// Device-clock span of a launch (WfFrameStats::trace_dev_ms): block 0 records the start, the last
// wave of every block its end, as a max on its XCD's line (`done`: an LDS wave counter zeroed
// before the block's first barrier); ts < 0 (host-driven rounds, or spans off: rt_set_device_spans)
// records nothing.  C3g, four slots: one 64-bit atomic per wave on one line cost the frame 2.5 %
// (8.67-8.71 -> 8.47-8.50 Grays/s), per block on per-XCD lines still ~1 % (8.58-8.62), so the
// spans are off unless asked for.
__device__ __forceinline__ void ts_start(const WfParams& Q, int ts) {
    if (ts >= 0 && blockIdx.x == 0 && threadIdx.x == 0) Q.W.tstamp[ts * kTsStride] = __builtin_amdgcn_s_memrealtime();
}
__device__ __forceinline__ void ts_end(const WfParams& Q, int ts, uint32_t* done) {
    if (ts < 0 || lane_id() != 0) return;
    if (atomicAdd(done, 1u) == (blockDim.x + 63u) / 64u - 1u)
        atomicMax(&Q.W.tstamp[ts * kTsStride + kTsLine * (1 + (int)(blockIdx.x % (uint32_t)kTsXcds))],
                  (unsigned long long)__builtin_amdgcn_s_memrealtime());
}

// dev_ctl statistics: rounds run, wf_trace launches run, rays they traced
__device__ __forceinline__ void stat_add(const WfParams& Q, int word, uint32_t v) {
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&Q.W.counts[kWfStat + word], v);
}
__device__ __forceinline__ bool tail_mode(const WfParams& Q) {
    return Q.dev_ctl && __builtin_amdgcn_readfirstlane(Q.W.counts[cslot(kCntTailMode)]) != 0u;
}

__device__ __forceinline__ bool likely_long(const PathRegs& p) {
    return p.tpass > 0 || p.bounce < p.step;
}

// A path's state between launches: its accumulator here (indexed by path id), its throughput
// colour and bounce / step counters in the queue entry of its next ray (qc, d.w), its pixel,
// sample and Halton index recomputed from the path id (path_meta); only the extra-sample paths,
// whose ids do not encode their pixel, keep them in p_meta.
__device__ __forceinline__ void init_path(const WfParams& Q, uint32_t pid, uint32_t pix, int sample, uint32_t hidx) {
    Q.W.p_accum[pid] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (pid >= Q.base_paths) Q.W.p_meta[pid] = make_uint4(pix, (uint32_t)sample, 0u, hidx);
}


// SKIPS: a kernel that shades, with the shadow rays its steps resolved themselves (rt_kernels.h)
template <bool SKIPS = false>
__device__ __forceinline__ void flush_counters(const FrameParams& P, uint32_t closest, uint32_t shadow, uint32_t paths,
                                               const TraceCounters& tc, bool count, bool overflow,
                                               bool trace_kernel = false, uint32_t root_retired = 0, uint32_t dark = 0,
                                               uint32_t root_unoccluded = 0, uint32_t shade_skipped = 0) {
    block_flush_counters<SKIPS>(P.counters, closest, shadow, count ? tc.nodes : 0u, count ? tc.tris : 0u, paths, overflow,
                                trace_kernel, count ? tc.lds_nodes : 0u, root_retired, dark, root_unoccluded, shade_skipped);
}
// A producer's end: the closest-hit rays it retired on root mask 0 (`retired`, a wave-uniform count)
// count where wf_trace would have counted them as misses: closest rays, and in a counting frame one
// node visit each (the root) of the traversal launches.  The shadow rays wf_shade resolved itself
// (`dark`, `unoccluded`: wave-uniform counts by class) count where connect would have counted
// them, as shadow rays; they add no node visit and no triangle test, since none happens.
template <bool SKIPS = false>
__device__ __forceinline__ void flush_producer(const FrameParams& P, const WfParams& Q, uint32_t retired, uint32_t paths,
                                               uint32_t dark = 0, uint32_t unoccluded = 0) {
    const bool l0 = lane_id() == 0;
    const uint32_t r = l0 ? retired : 0u, dk = l0 ? dark : 0u, un = l0 ? unoccluded : 0u;
    const TraceCounters tc{r, 0, 0};
    flush_counters<SKIPS>(P, r, dk + un, paths, tc, Q.count != 0, false, true, r, dk, un, dk + un);
}

// per-pixel outputs of a shade step (depth / motion / G-buffer, :342-389, :506-515)
// (depth and motion: the hit is recorded and wf_motion evaluates it after the pass)
__device__ __forceinline__ void write_pixel_outputs(const FrameParams& P, uint32_t pix, const StepResult& r, const Hit& h,
                                                    bool full) {
    if (r.primary) P.prim_hit[pix] = make_uint4(h.id, __float_as_uint(h.u), __float_as_uint(h.v), 0u);
    if (full && r.gbuf && P.gbuffer) {
        size_t plane = (size_t)P.U.width * P.U.height;
        P.gbuffer[pix] = r.g0;
        P.gbuffer[plane + pix] = r.g1;
        P.gbuffer[2 * plane + pix] = r.g2;
        P.gbuffer[3 * plane + pix] = r.g3;
    }
}

// ---- root words (rt_device.h root_word, rt_trav.h trav_start_root) -------------------------------
// Producers: what their root test reads, once per block into LDS (call before a block barrier that
// comes before the first producer_root_word, such as load_tabs'); the mask then costs no memory
// access per ray.  RT_ROOT_TIGHT: the exact boxes of the root's children; else the root's five words.
#if RT_ROOT_TIGHT
using RootLds = RootBoxes;
#else
using RootLds = NodeWords;
#endif
__device__ __forceinline__ void stage_root(const DevScene& S, RootLds* lds_root) {
    static_assert(sizeof(NodeWords) == sizeof(Bvh8Node) && offsetof(NodeWords, h1) == 16 && offsetof(NodeWords, qx) == 32,
                  "NodeWords: the node's own layout");
    const uint32_t* src = RT_ROOT_TIGHT ? reinterpret_cast<const uint32_t*>(S.root_box) : reinterpret_cast<const uint32_t*>(S.nodes8);
    if (threadIdx.x < sizeof(RootLds) / 4u) reinterpret_cast<uint32_t*>(lds_root)[threadIdx.x] = src[threadIdx.x];
}
__device__ __forceinline__ uint32_t producer_root_word(const RootLds& root, f3 o, f3 d, float tmax) {
#if RT_ROOT_TIGHT
    return root_word_tight(root, o, d, tmax);
#else
    return root_word(root, o, d, tmax);
#endif
}
// A closest-hit ray its producer retires: a valid word with mask 0 is a proven miss (its first
// trav_step would return one), so the ray is not enqueued and its path ends here.
__device__ __forceinline__ bool root_retires(uint32_t word) { return RT_ROOT_TIGHT && word == kRootValid; }
// A shadow ray wf_shade resolves: the same word proves it unoccluded (connect's first trav_step would
// end it with no hit), so wf_shade adds its contribution itself and appends no shadow entry.
#ifndef RT_SHADE_UNOCCLUDED
#define RT_SHADE_UNOCCLUDED RT_ROOT_TIGHT   // 0: such a ray keeps its shadow entry and connect ends it in one iteration
#endif
__device__ __forceinline__ bool root_unoccluded(uint32_t word) { return RT_SHADE_UNOCCLUDED && word == kRootValid; }
// Consumers: the root's header words, the same for every lane (scalar registers).
__device__ __forceinline__ RootHead load_root_head(const DevScene& S) {
    const uint32_t* w = reinterpret_cast<const uint32_t*>(S.nodes8);
    RootHead H;
    H.ew = __builtin_amdgcn_readfirstlane(w[3]);
    H.h1.x = __builtin_amdgcn_readfirstlane(w[4]);
    H.h1.y = __builtin_amdgcn_readfirstlane(w[5]);
    H.h1.z = __builtin_amdgcn_readfirstlane(w[6]);
    return H;
}

}  // namespace

// ---- base paths ----------------------------------------------------------------------------------------
// Halton index of sample s of pixel pix in this frame (:263-270)
__device__ __forceinline__ uint32_t base_hidx(const FrameParams& P, int spp, uint32_t pix, int s) {
    const Uniforms& U = P.U;
    const int maxExtra = (U.enableMotionAdaptiveSampling != 0) ? max(U.motionSamplingMaxExtraSamples, 0) : 0;
    const int frameOffset = (int)U.frameIndex * (spp + maxExtra) + s;
    return (uint32_t)(int)(P.random[pix] + (unsigned)frameOffset);
}
// Path pid of the base pass (own pixel pid / spp, sample pid % spp): its pixel, sample, Halton index
// (:263-270) and primary ray (:270-292).  False for a path of a tile pixel outside the image.
__device__ __forceinline__ bool base_path(const FrameParams& P, const WfParams& Q, const ShadeTabs& halton, uint32_t pid,
                                          uint32_t& pix, int& s, uint32_t& hidx, f3& o, f3& d) {
    const Uniforms& U = P.U;
    const uint32_t i = fdiv(pid, Q.px.spp_div);
    s = (int)(pid - i * Q.px.spp_div.d);
    int px, py;
    own_pixel(Q.px, i, px, py);
    if (px >= U.width || py >= U.height) return false;
    pix = (uint32_t)py * (uint32_t)U.width + (uint32_t)px;
    hidx = base_hidx(P, Q.spp, pix, s);
    primary_ray(U, halton, px, py, (int)hidx, o, d);
    return true;
}
// (pixel, sample, Halton index) of path pid: a base path's from its id, as wf_generate made them;
// an extra-sample path's from p_meta (wf_extra)
__device__ __forceinline__ uint3 path_meta(const FrameParams& P, const WfParams& Q, uint32_t pid) {
    if (pid >= Q.base_paths) {
        const uint4 m = Q.W.p_meta[pid];
        return make_uint3(m.x, m.y, m.w);
    }
    const uint32_t i = fdiv(pid, Q.px.spp_div);
    const int s = (int)(pid - i * Q.px.spp_div.d);
    int px, py;
    own_pixel(Q.px, i, px, py);
    const uint32_t pix = (uint32_t)py * (uint32_t)P.U.width + (uint32_t)px;
    return make_uint3(pix, (uint32_t)s, base_hidx(P, Q.spp, pix, s));
}
// Queue entry {o, d} -> the path it carries: its id (o.w), its (pixel, sample, state bits, Halton
// index) and its registers.  colour(): the entry's throughput colour, read only past state 0 (the
// primary ray's is 1).  A continuation ray past bounce 0 carries its Halton index in the colour's w:
// the pixel and sample (and the per-pixel random offset behind them) are read only at bounce 0
// (:342-389).  read_accum: start from the stored accumulator, else from zero.
template <typename Colour>
__device__ __forceinline__ void load_path(const FrameParams& P, const WfParams& Q, const float4& o, const float4& d,
                                          Colour colour, bool read_accum, uint32_t& pid, uint4& meta, PathRegs& p) {
    pid = __float_as_uint(o.w);
    const uint32_t state = __float_as_uint(d.w);
    const float4 c = state == 0u ? make_float4(1.0f, 1.0f, 1.0f, 0.0f) : colour();
    const PathState st = unpack_state(state);
    if (st.bounce != 0) {
        meta = make_uint4(0u, 1u, state, __float_as_uint(c.w));
    } else {
        const uint3 pm = path_meta(P, Q, pid);
        meta = make_uint4(pm.x, pm.y, state, pm.z);
    }
    const float4 a = read_accum ? Q.W.p_accum[pid] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    p.color = mk3(c.x, c.y, c.z);
    p.accum = mk3(a.x, a.y, a.z);
    p.bounce = st.bounce;
    p.tpass = st.tpass;
    p.step = st.step;
}
// Per-pixel defaults, written by the pixel's sample-0 path (:252-261).
__device__ __forceinline__ void init_pixel(const FrameParams& P, uint32_t pix) {
    P.depth[pix] = 1.0e8f;
    P.motion[pix] = make_float2(0.0f, 0.0f);
    P.prim_hit[pix] = make_uint4(0xffffffffu, 0u, 0u, 0u);
    if (P.gbuffer) {
        const size_t plane = (size_t)P.U.width * P.U.height;
        const float4 z = make_float4(0, 0, 0, 0);
        P.gbuffer[pix] = z;
        P.gbuffer[plane + pix] = z;
        P.gbuffer[2 * plane + pix] = z;
        P.gbuffer[3 * plane + pix] = z;
    }
}
// ---- generate -------------------------------------------------------------------------------------
// (A first round fused with generate -- extend making the primary rays at refill, shade starting
// the path state -- was measured slower)
__global__ void __launch_bounds__(kBlock) wf_generate(DevScene S, const FrameParams* __restrict__ Pp, WfParams Q) {
    const FrameParams& P = *Pp;   // per-frame parameters in device memory
    __shared__ HaltonDim lds_halton[kHaltonLds];
    __shared__ BlockAlloc ba;
    __shared__ RootLds lds_root;
    stage_root(S, &lds_root);
    const ShadeTabs halton = load_tabs(S, lds_halton, nullptr);   // no shading: Halton only
    const Uniforms& U = P.U;
    const int spp = Q.spp;
    const int shard = blockIdx.x & (kShards - 1);
    float4* qout = Q.W.q[0] + 2 * (size_t)shard * Q.seg_cap;
    uint32_t* qrout = Q.W.qr[0] + (size_t)shard * Q.seg_cap;
    uint32_t n_paths = 0, n_retired = 0;   // n_retired: wave-uniform
    const uint32_t total = Q.base_paths;
    if (Q.dev_ctl && blockIdx.x == 0 && threadIdx.x == 0) Q.W.counts[cslot(kCntFinishQ)] = (uint32_t)Q.finish_q;
    for (uint32_t base = blockIdx.x * kBlock; base < total; base += gridDim.x * kBlock) {
        uint32_t pid = base + threadIdx.x;
        int s = 0;
        uint32_t pix = 0, hidx = 0;
        f3 o = mk3(0, 0, 0), d = mk3(0, 0, 0);
        const bool valid = pid < total && base_path(P, Q, halton, pid, pix, s, hidx, o, d);
        if (valid) {
            init_path(Q, pid, pix, s, hidx);
            if (s == 0) init_pixel(P, pix);
            n_paths++;
        }
        bool live = valid && U.maxBounces > 0;
        // the primary ray's root word; a ray that leaves the scene is never enqueued
        const uint32_t rw = live ? producer_root_word(lds_root, o, d, INFINITY) : 0u;
        const bool dead = live && root_retires(rw);
        n_retired += (uint32_t)__popcll(__ballot(dead));
        live = live && !dead;
        uint32_t slot = block_alloc(live, &Q.W.counts[cslot(shard)], ba);
        if (live) {
            qout[2 * slot] = make_float4(o.x, o.y, o.z, __uint_as_float(pid));
            qout[2 * slot + 1] = make_float4(d.x, d.y, d.z, 0.0f);
            qrout[slot] = rw;
        }
    }
    flush_producer(P, Q, n_retired, n_paths);
}

// ---- shade -------------------------------------------------------------------------------------------
// SORTED: the input is the hit-sorted array (wf_sort_scatter; misses already dropped) and the
// blocks of XCD k (blockIdx % 8) shade the k-th eighth of it, so one XCD's L2 serves one scene
// region and the rays / shadow rays it appends to its queue shard stay grouped by region for
// the next extend / connect launches (which hand shard k's range to XCD k).
// The radiance instances are held at five waves per SIMD (96 VGPRs): left to itself the compiler takes
// 102 for <false, false> and drops to four.
template <bool FULL, bool SORTED>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(FULL ? 3 : 5, FULL ? 3 : 5)))
wf_shade(DevScene S, const FrameParams* __restrict__ Pp, WfParams Q, int cur) {
    const FrameParams& P = *Pp;   // per-frame parameters in device memory
    __shared__ HaltonDim lds_halton[kHaltonLds];
    __shared__ MatRec lds_mat[kMatLds];
    __shared__ float4 lds_inst[3 * kInstLds];
    __shared__ Light lds_light[kLightLds];
    __shared__ SpotCone lds_spot[kLightLds];
    __shared__ BlockAllocOct bao;
    __shared__ RootLds lds_root;
    if (tail_mode(Q)) return;
    stage_root(S, &lds_root);
    const ShadeTabs halton = load_tabs(S, lds_halton, lds_mat, lds_inst, lds_light, lds_spot, P.U.lightCount);
    const Uniforms& U = P.U;
    const int next = 1 - cur;
    const int shard = blockIdx.x & (kShards - 1);
    const QueueShards qs = load_queue(Q.W.counts, cur, Q.seg_cap);
    const float4* qin = Q.W.q[cur];
    float4* qout = Q.W.q[next] + 2 * (size_t)shard * Q.seg_cap;
    float4* qcout = Q.W.qc[next] + (size_t)shard * Q.seg_cap;
    uint32_t* qrout = Q.W.qr[next] + (size_t)shard * Q.seg_cap;
    float4* sqout = Q.W.sq + 3 * (size_t)shard * Q.seg_cap;
    f2 zero2;
    zero2.x = 0.0f;
    zero2.y = 0.0f;
    // the blocks of XCD k (blockIdx % 8, the grid is a multiple of 8: grid_for) take queue shard k,
    // which XCD k's extend launch traced (unsorted), or the k-th eighth of the sorted array
    uint32_t beg = (blockIdx.x >> 3) * kBlock, end = 0, ebase = 0, lk = 0;
    const uint32_t stride = (gridDim.x >> 3) * kBlock;
    if (SORTED) {
        const uint32_t n = __builtin_amdgcn_readfirstlane(Q.W.counts[cslot(kCntSorted)]);
        beg += (uint32_t)(((uint64_t)n * (uint32_t)shard) / kShards);
        end = (uint32_t)(((uint64_t)n * (uint32_t)(shard + 1)) / kShards);
    } else {
        #pragma unroll
        for (int j = 0; j < kShards; ++j)
            if (j == shard) {
                lk = qs.L[j];
                end = qs.L[j] + qs.S[j];
            }
        ebase = (uint32_t)shard * Q.seg_cap;
    }
    // Unsorted: a missed ray ends its path and adds nothing (:321-322), so it gets no lane of a shading
    // pass.  The block walks its batches of kBlock queue entries in order, reads each entry's hit
    // record and compacts the hits (entry index and record, by ballot and a prefix over the waves)
    // into an LDS ring; it shades once kBlock hits wait, or what is left after its last batch.  The
    // hits keep the queue's order, so the rays and shadow rays appended stay grouped as before.
    // A fill adds at most kBlock to fewer than kBlock waiting: the ring holds 2 * kBlock.
    constexpr uint32_t kRing = 2 * kBlock;
    __shared__ uint32_t ring_e[SORTED ? 1 : kRing];
    __shared__ float4 ring_h[SORTED ? 1 : kRing];
    __shared__ uint32_t ring_w[2][kBlock / 64];   // the waves' hit counts of a fill (double-buffered: one barrier per fill)
    uint32_t head = 0, pending = 0, fills = 0;    // block-uniform
    uint32_t n_retired = 0;                       // wave-uniform: continuation rays retired on root mask 0
    uint32_t n_dark = 0, n_unoccluded = 0;        // wave-uniform: shadow rays resolved here (±0 contribution; root mask 0)
    uint32_t base = beg;
    while (true) {
        uint32_t g = base + threadIdx.x;
        bool valid;
        uint32_t slot = 0;
        if (SORTED) {
            if (base >= end) break;
            valid = g < end;
            base += stride;
        } else {
            while (pending < (uint32_t)kBlock && base < end) {
                g = base + threadIdx.x;
                uint32_t e = 0;
                float4 hv = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                bool hit = false;
                if (g < end) {
                    e = ebase + seg_pos(g, lk, Q.seg_cap);
                    hv = ld_stream(&Q.W.hits[e]);
                    hit = __float_as_uint(hv.y) != 0xffffffffu;
                }
                const unsigned long long m = __ballot(hit);
                uint32_t off, tot;
                block_prefix<kBlock / 64>(lane_id() == 0, (uint32_t)__popcll(m), ring_w[fills & 1u], off, tot);
                if (hit) {
                    const uint32_t s = (head + pending + off + mbcnt64(m)) & (kRing - 1u);
                    ring_e[s] = e;
                    ring_h[s] = hv;
                }
                pending += __builtin_amdgcn_readfirstlane(tot);   // the same in every thread: the loops stay uniform
                ++fills;
                base += stride;
            }
            if (pending == 0u) break;
            // the ring's new entries are written; the slots read below are free for the next fill
            // once every thread has passed block_alloc3_oct's barriers
            __syncthreads();
            const uint32_t n = min(pending, (uint32_t)kBlock);
            valid = threadIdx.x < n;
            slot = (head + threadIdx.x) & (kRing - 1u);
            head = (head + n) & (kRing - 1u);
            pending -= n;
        }
        StepResult r;
        r.next = false;
        r.shadow = false;
        r.dark = false;
        bool lit = false;               // the step's shadow ray is proven unoccluded (root mask 0)
        uint32_t rws = 0;               // the shadow ray's root word
        uint32_t pid = 0, nstate = 0;   // nstate, ncol: the continuation's state bits and colour
        bool front = true;              // the continuation goes to the queue front (likely_long)
        f3 rayO = mk3(0, 0, 0), rayD = mk3(0, 0, 0);
        float4 ncol = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (valid) {
            float4 o, d, hv;
            size_t ce = 0;   // the entry's colour: sorted[4g + 3] / qc[cur][e]
            if (SORTED) {
                o = Q.W.sorted[4 * (size_t)g];
                d = Q.W.sorted[4 * (size_t)g + 1];
                hv = Q.W.sorted[4 * (size_t)g + 2];
                ce = 4 * (size_t)g + 3;
            } else {
                const uint32_t e = ring_e[slot];
                hv = ring_h[slot];
                o = ld_stream(&qin[2 * (size_t)e]);
                d = ld_stream(&qin[2 * (size_t)e + 1]);
                ce = e;
            }
            Hit h;
            h.t = hv.x;
            h.id = __float_as_uint(hv.y);
            h.u = hv.z;
            h.v = hv.w;
            pid = __float_as_uint(o.w);
            if (!SORTED || h.id != 0xffffffffu) {   // sorted: dropped by the sort already; unsorted: never in the ring
                // FULL=false: shade_step only adds color * emission to accum (:585), so it runs on a
                // zero accumulator and the stored one is read and updated only when that term is
                // non-zero (accum is never -0, so a + (0 + x) == a + x bit for bit); FULL (debug
                // modes assign accum) reads it first
                uint4 meta;
                PathRegs p;
                load_path(P, Q, o, d, [&]() { return SORTED ? Q.W.sorted[ce] : ld_stream(&Q.W.qc[cur][ce]); }, FULL, pid,
                          meta, p);
                const f3 a = p.accum;
                int sample = (int)meta.y;
                rayO = ld3(o);
                rayD = ld3(d);
                shade_step<FULL, false>(S, U, halton, (int)meta.w, sample, rayO, rayD, h, p, sample == 0 && p.step == 0,
                                 zero2, false, zero2, r);
                write_pixel_outputs(P, meta.x, r, h, FULL);
                nstate = pack_state(p.bounce, p.tpass, p.step);
                front = likely_long(p);
                ncol = make_float4(p.color.x, p.color.y, p.color.z, __uint_as_float(meta.w));   // w: Halton index
                // A shadow ray with root mask 0 is proven unoccluded: its contribution is added here,
                // in connect's order (:741-743 after :585: (stored + emission) + contribution), and
                // it gets no shadow entry.  (A dark one has neither: shade_step cleared r.shadow.)
                rws = r.shadow ? producer_root_word(lds_root, r.so, r.sd, r.stmax) : 0u;
                lit = r.shadow && root_unoccluded(rws);
                r.shadow = r.shadow && !lit;
                // radiance only changes on emissive hits (:585-586) and by such a contribution: skip
                // the read and the store otherwise (no emission: s + (+0) == s, s is never -0)
                if (lit || __float_as_uint(p.accum.x) != __float_as_uint(a.x) || __float_as_uint(p.accum.y) != __float_as_uint(a.y) ||
                    __float_as_uint(p.accum.z) != __float_as_uint(a.z)) {
                    if (!FULL) {
                        const float4 s = Q.W.p_accum[pid];
                        p.accum = mk3(s.x + p.accum.x, s.y + p.accum.y, s.z + p.accum.z);
                    }
                    if (lit) p.accum = p.accum + r.contrib;
                    Q.W.p_accum[pid] = make_float4(p.accum.x, p.accum.y, p.accum.z, 0.0f);
                }
            }
        }
        // each ray with its root word: the root's 8-wide test here, at this kernel's lane
        // utilisation, and the traversal starts from its result (trav_start_root).  A continuation
        // ray that leaves the scene is never enqueued: its path ends as after a miss record.
        const uint32_t rwn = r.next ? producer_root_word(lds_root, rayO, rayD, INFINITY) : 0u;
        const bool dead = r.next && root_retires(rwn);
        n_retired += (uint32_t)__popcll(__ballot(dead));
        r.next = r.next && !dead;
        n_dark += (uint32_t)__popcll(__ballot(r.dark));
        n_unoccluded += (uint32_t)__popcll(__ballot(lit));
        const bool pr[3] = {r.shadow, r.next && front, r.next && !front};
        uint32_t* const ctr[3] = {&Q.W.counts[cslot(kCntShadowQ + shard)], &Q.W.counts[cslot(next * kShards + shard)],
                                  &Q.W.counts[cslot(kCntBack + next * kShards + shard)]};
        uint32_t slots[3];
        // continuation rays grouped by direction octant inside the block's range (round 5: +-0, kept)
        const uint32_t oct = (rayD.x < 0.0f ? 1u : 0u) | (rayD.y < 0.0f ? 2u : 0u) | (rayD.z < 0.0f ? 4u : 0u);
        block_alloc3_oct(pr, oct, ctr, bao, slots);
        const uint32_t ns = slots[0], nr = front ? slots[1] : Q.seg_cap - 1u - slots[2];
        if (r.shadow) {
            sqout[3 * (size_t)ns] = make_float4(r.so.x, r.so.y, r.so.z, __uint_as_float(pid));
            sqout[3 * (size_t)ns + 1] = make_float4(r.sd.x, r.sd.y, r.sd.z, r.stmax);
            sqout[3 * (size_t)ns + 2] = make_float4(r.contrib.x, r.contrib.y, r.contrib.z, __uint_as_float(rws));
        }
        if (r.next) {
            qout[2 * (size_t)nr] = make_float4(rayO.x, rayO.y, rayO.z, __uint_as_float(pid));
            qout[2 * (size_t)nr + 1] = make_float4(rayD.x, rayD.y, rayD.z, __uint_as_float(nstate));
            qcout[nr] = ncol;
            qrout[nr] = rwn;
        }
    }
    flush_producer<true>(P, Q, n_retired, 0, n_dark, n_unoccluded);
}

// ---- hit sort (between extend and shade) -------------------------------------------------------------
// A counting sort of the extend queue's hits by key (the bin of the hit triangle's BVH leaf slot,
// S.tri_bin; leaf order is spatially coherent, so a bin is one scene region), in three launches: per-block histograms, a scan of each bin's row of block counts, and a
// scatter that writes {o, d, hit} of every hit to its bin's range.  Misses are dropped (their
// paths end, :321-322).  The order inside a bin is arbitrary; per-path results do not depend on
// the order paths are shaded in, so the output stays bit-identical.
// block b's share of the dense queue index range (the same in hist and scatter)
__device__ __forceinline__ void sort_range(uint32_t n, uint32_t& beg, uint32_t& end) {
    beg = (uint32_t)(((uint64_t)n * blockIdx.x) / kSortBlocks);
    end = (uint32_t)(((uint64_t)n * (blockIdx.x + 1)) / kSortBlocks);
}

// sort key of queue entry e: kNoKey for a miss, else the leaf bin at Q.sort_bins resolution
__device__ __forceinline__ uint32_t sort_key(const DevScene& S, const WfParams& Q, uint32_t e, uint32_t shift) {
    const uint32_t id = __float_as_uint(Q.W.hits[e].y);
    return id == 0xffffffffu ? kNoKey : ((uint32_t)S.tri_bin[id] >> shift);
}

__global__ void __launch_bounds__(kSortThreads) wf_sort_hist(DevScene S, WfParams Q, int cur) {
    __shared__ uint32_t h[kSortMaxBins];
    if (tail_mode(Q)) return;
    const uint32_t shift = __builtin_ctz(kSortMaxBins) - __builtin_ctz(Q.sort_bins);
    const uint32_t K = Q.sort_bins;
    const QueueShards qs = load_queue(Q.W.counts, cur, Q.seg_cap);
    for (uint32_t k = threadIdx.x; k < K; k += kSortThreads) h[k] = 0;
    __syncthreads();
    uint32_t beg, end;
    sort_range(queue_len(qs), beg, end);
    for (uint32_t g = beg + threadIdx.x; g < end; g += kSortThreads) {
        const uint32_t k = sort_key(S, Q, dense_entry(qs, g, Q.seg_cap), shift);
        if (k != kNoKey) atomicAdd(&h[k], 1u);
    }
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < K; k += kSortThreads) Q.W.sort_table[(size_t)k * kSortBlocks + blockIdx.x] = h[k];
}

// one block per bin: exclusive scan of the bin's kSortBlocks block counts (in place) + bin total
__global__ void __launch_bounds__(kSortBlocks) wf_sort_rowscan(WfParams Q) {
    __shared__ uint32_t w[kSortBlocks / 64];
    if (tail_mode(Q)) return;
    uint32_t* row = Q.W.sort_table + (size_t)blockIdx.x * kSortBlocks;
    const uint32_t v = row[threadIdx.x];
    const uint32_t incl = wave_incl_scan(v);
    uint32_t base, total;
    block_prefix<kSortBlocks / 64>(lane_id() == 63, incl, w, base, total);
    row[threadIdx.x] = base + incl - v;
    if (threadIdx.x == kSortBlocks - 1) Q.W.sort_total[blockIdx.x] = total;
}

__global__ void __launch_bounds__(kSortThreads) wf_sort_scatter(DevScene S, WfParams Q, int cur) {
    __shared__ uint32_t off[kSortMaxBins];
    if (tail_mode(Q)) return;
    const uint32_t shift = __builtin_ctz(kSortMaxBins) - __builtin_ctz(Q.sort_bins);
    __shared__ uint32_t w[kSortThreads / 64];
    const uint32_t K = Q.sort_bins, per = K / kSortThreads;   // 1, 2 or 4 bins per thread
    const QueueShards qs = load_queue(Q.W.counts, cur, Q.seg_cap);
    // bin starts: exclusive scan of the bin totals, plus this block's offset inside each bin
    uint32_t loc[kSortMaxBins / kSortThreads];
    uint32_t s = 0;
    for (uint32_t i = 0; i < per; ++i) {
        loc[i] = s;
        s += Q.W.sort_total[threadIdx.x * per + i];
    }
    const uint32_t incl = wave_incl_scan(s);
    uint32_t base, total;
    block_prefix<kSortThreads / 64>(lane_id() == 63, incl, w, base, total);
    const uint32_t excl = base + incl - s;
    for (uint32_t i = 0; i < per; ++i) {
        const uint32_t k = threadIdx.x * per + i;
        off[k] = excl + loc[i] + Q.W.sort_table[(size_t)k * kSortBlocks + blockIdx.x];
    }
    if (blockIdx.x == 0 && threadIdx.x == kSortThreads - 1) Q.W.counts[cslot(kCntSorted)] = total;
    __syncthreads();
    const float4* qin = Q.W.q[cur];
    uint32_t beg, end;
    sort_range(queue_len(qs), beg, end);
    for (uint32_t g = beg + threadIdx.x; g < end; g += kSortThreads) {
        const uint32_t e = dense_entry(qs, g, Q.seg_cap);
        const float4 hv = Q.W.hits[e];
        const uint32_t id = __float_as_uint(hv.y);
        if (id == 0xffffffffu) continue;
        const uint32_t pos = atomicAdd(&off[(uint32_t)S.tri_bin[id] >> shift], 1u);
        const float4 o = qin[2 * (size_t)e], d = qin[2 * (size_t)e + 1];
        Q.W.sorted[4 * (size_t)pos] = o;
        Q.W.sorted[4 * (size_t)pos + 1] = d;
        Q.W.sorted[4 * (size_t)pos + 2] = hv;
        if (__float_as_uint(d.w) != 0u) Q.W.sorted[4 * (size_t)pos + 3] = Q.W.qc[cur][e];   // state 0: colour 1
    }
}

// connect: the accumulation of the unoccluded shadow rays of a wave, batched (one lane per pending
// entry: its path id and contribution from the shadow queue, then accum += contribution, :741-743)
// so the wave waits for these dependent loads once per up to 64 rays, not once per finishing step.
// A path has one shadow ray per connect launch, so the order of the additions is unchanged.
__device__ __forceinline__ void connect_flush(const WfParams& Q, const float4* qin, uint32_t* pend, uint32_t& npend) {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const uint32_t lane = lane_id();
    if (lane < npend) {
        const uint32_t e = pend[lane];
        const float4 o4 = qin[3 * (size_t)e];
        const float4 c = qin[3 * (size_t)e + 2];
        const uint32_t pid = __float_as_uint(o4.w);
        const float4 a = Q.W.p_accum[pid];
        Q.W.p_accum[pid] = make_float4(a.x + c.x, a.y + c.y, a.z + c.z, 0.0f);
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
    npend = 0;
}

// ---- persistent traversal with per-lane refill (extend: ANY = false, connect: ANY = true) -----------
// The grid is the resident capacity.  Each XCD (blockIdx % 8) owns queue shard k (what its own shade blocks appended) and hands
// it out in chunks of Q.chunk rays, one atomic per chunk.  Every iteration advances each lane of a
// wave by one traversal step (trav_step); a lane whose query ended takes the next ray of the
// wave's chunk once at least Q.refill_min lanes are idle.  A wave therefore runs ~(steps of its
// rays) / 64 iterations instead of (slowest ray) x (rays per lane).
template <bool ANY, bool COUNT>
#ifndef RT_EXTEND_WAVES
#define RT_EXTEND_WAVES 8
#endif
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(ANY ? 8 : RT_EXTEND_WAVES, ANY ? 8 : RT_EXTEND_WAVES)))
wf_trace(DevScene S, const FrameParams* __restrict__ Pp, WfParams Q, int cur, int ts) {
    const FrameParams& P = *Pp;   // per-frame parameters in device memory
    __shared__ int lds_stack[kStackSize * kBlock];
    int* stack = &lds_stack[threadIdx.x];
    if (Q.dev_ctl) {
        // device-side round control: extend decides (uniformly, from the counters) whether this
        // round runs in bulk or the rest of the pass goes to the finish launch
        const bool tm = tail_mode(Q);
        if (ANY) {
            if (tm) return;
        } else {
            if (tm || queue_len(load_queue(Q.W.counts, cur, Q.seg_cap)) < Q.tail) {
                if (!tm && blockIdx.x == 0 && threadIdx.x == 0) {
                    Q.W.counts[cslot(kCntTailMode)] = 1u;
                    Q.W.counts[cslot(kCntFinishQ)] = (uint32_t)cur;
                }
                return;
            }
        }
    }
    __shared__ uint32_t ts_done;
    if (threadIdx.x == 0) ts_done = 0u;
    ts_start(Q, ts);
    __syncthreads();
    // the shadow queue is one-sided, a ray queue two-sided (front / back parts)
    const uint32_t n = ANY ? load_prefix(Q.W.counts + cslot(kCntShadowQ)).end[kShards - 1]
                           : queue_len(load_queue(Q.W.counts, cur, Q.seg_cap));
    if (Q.dev_ctl) {
        stat_add(Q, kStatTraceRays, n);
        stat_add(Q, kStatTraceLaunches, 1u);
        if (!ANY) {
            stat_add(Q, kStatRounds, 1u);
            stat_add(Q, kStatExtendRays, n);
        }
    }
    if (!ANY && blockIdx.x == 0 && threadIdx.x < 3 * kShards) {  // reset the queues shade / connect fill
        const int next = 1 - cur;
        const uint32_t k = threadIdx.x & (kShards - 1), part = threadIdx.x / kShards;
        Q.W.counts[cslot(part == 0 ? next * kShards + k : part == 1 ? kCntShadowQ + k : kCntBack + next * kShards + k)] = 0;
    }
    // chunk counters of the OTHER traversal kind are reset here for its next launch (extend and
    // connect alternate; the frame start zeroes both)
    if (blockIdx.x == 0 && threadIdx.x < kShards)
        Q.W.counts[cslot((ANY ? kCntChunkExtend : kCntChunkConnect) + threadIdx.x)] = 0;
    const float4* qin = ANY ? Q.W.sq : Q.W.q[cur];
    const int qstride = ANY ? 3 : 2;
    const RootHead root = load_root_head(S);
    // chunks of this XCD's part of the queue, grabbed with one atomic per chunk
    const uint32_t xcd = blockIdx.x & 7u;
    uint32_t* const chunk_ctr = Q.W.counts + cslot((ANY ? kCntChunkConnect : kCntChunkExtend) + (int)xcd);
    // XCD k traverses queue shard k, the segment its own shade blocks (blockIdx % 8 == k) appended:
    // entry = k * seg_cap + g, no per-lane search of the shard prefix
    // shard xcd's entries and its front part (two scalar loads)
    uint32_t xl, xend;
    if (ANY) {
        xl = xend = min(__builtin_amdgcn_readfirstlane(Q.W.counts[cslot(kCntShadowQ + (int)xcd)]), Q.seg_cap);
    } else {
        xl = min(__builtin_amdgcn_readfirstlane(Q.W.counts[cslot(cur * kShards + (int)xcd)]), Q.seg_cap);
        xend = xl + min(__builtin_amdgcn_readfirstlane(Q.W.counts[cslot(kCntBack + cur * kShards + (int)xcd)]),
                        Q.seg_cap - xl);
    }
    // (round 3; before, XCD k took the k-th eighth of the dense queue and every refilling lane
    // searched the prefix for its entry: 7.49 -> 7.56 Grays/s)
    const uint32_t xbeg = 0, ebase = xcd * Q.seg_cap;
    uint32_t wnext = 0, wend = 0;
    bool exhausted = false;

    TraceCounters tc{0, 0, 0};
    bool overflow = false;
    uint32_t rays = 0;
    bool active = false;
    uint32_t e = 0;
    Trav T;
    trav_start(T, mk3(0, 0, 0), mk3(1, 0, 0), 0.0f);
    uint32_t steps = 0;   // COUNT: iterations the current ray has taken
    __shared__ uint32_t lds_pend_all[ANY ? kBlock : 1];
    uint32_t* const lds_pend = &lds_pend_all[ANY ? (threadIdx.x & ~63u) : 0u];   // the wave's 64 slots
    uint32_t npend = 0;   // wave-uniform

    while (true) {
        // refill idle lanes from the wave's chunk
        const unsigned long long idle = __ballot(!active);
        const bool refill = __popcll(idle) >= Q.refill_min || idle == ~0ull;
        if (wnext >= wend && !exhausted && refill) {
            uint32_t base = 0;
            if (lane_id() == 0) base = atomicAdd(chunk_ctr, (uint32_t)Q.chunk);
            base = xbeg + __builtin_amdgcn_readfirstlane(base);
            if (base >= xend) {
                exhausted = true;
            } else {
                wnext = base;
                wend = min(base + (uint32_t)Q.chunk, xend);
            }
        }
        if (idle != 0ull && wnext < wend && refill) {
            if (!active) {
                uint32_t g = wnext + mbcnt64(idle);
                if (g < wend) {
                    e = ebase + (ANY ? g : seg_pos(g, xl, Q.seg_cap));
                    float4 o4 = qin[(size_t)qstride * e];
                    float4 d4 = qin[(size_t)qstride * e + 1];
                    // the entry's root word: beside a ray's entry, or in the w of a shadow ray's third record
                    const uint32_t rw = ANY ? reinterpret_cast<const uint32_t*>(&qin[(size_t)qstride * e + 2])[3] : Q.W.qr[cur][e];
                    // a consumed word stands for the root's node visit; a mask of 0 ends in the
                    // lane's first trav_step below, which then does nothing (a miss / unoccluded)
                    if (trav_start_root(T, ld3(o4), ld3(d4), ANY ? d4.w : INFINITY, rw, root) && COUNT) tc.nodes++;
                    active = true;
                    rays++;
                    if (COUNT) steps = 0;
                }
            }
            wnext += (uint32_t)__popcll(idle);
        }
        if (__ballot(active) == 0ull) {
            if (ANY) connect_flush(Q, qin, lds_pend, npend);
            break;
        }
        bool acc = false;
        if (active) {
            if (COUNT) ++steps;
            if (trav_step<COUNT>(S, T, ANY, stack, tc, overflow, T.best)) {
                active = false;
                if (COUNT && Q.diag) {   // steps-per-ray histogram (log2 bins) of the counting frame
                    atomicAdd(&Q.W.counts[kWfDiagSteps + (ANY ? kDiagStepBins : 0) + (31 - __builtin_clz(steps))], 1u);
                    atomicMax(&Q.W.counts[kWfDiagSteps + 2 * kDiagStepBins + (ANY ? 1 : 0)], steps);
                }
                if (ANY) acc = !T.hit_any;
                else Q.W.hits[e] = make_float4(T.best, __uint_as_float(T.best_id), T.bu / T.bdet, T.bv / T.bdet);
            }
        }
        if (ANY) {   // unoccluded shadow rays: their entries wait in the wave's LDS list (connect_flush)
            const unsigned long long m = __ballot(acc);
            if (m != 0ull) {
                const uint32_t k = (uint32_t)__popcll(m);
                if (npend + k > 64u) connect_flush(Q, qin, lds_pend, npend);
                if (acc) lds_pend[npend + mbcnt64(m)] = e;
                npend += k;
            }
        }
    }
    ts_end(Q, ts, &ts_done);
    flush_counters(P, ANY ? 0 : rays, ANY ? rays : 0, 0, tc, COUNT, overflow, true);
}

// ---- finish: the remaining paths to completion, step-interleaved ---------------------------------------
// Below Q.tail live paths, one persistent launch runs every remaining path to completion.  Every
// lane advances by ONE traversal step per iteration (trav_step, closest-hit or shadow any-hit), as
// in wf_trace.  A lane whose closest-hit query ended waits in kReady; the wave shades all waiting
// lanes together once at least Q.shade_min of them wait (or no lane is traversing), then each
// continues with its shadow ray, its next ray, or the next path of the queue.  A wave therefore
// costs the sum of its own lanes' steps, not the sum over segments of its slowest lane's query:
// the glass paths left at the tail (up to ~23 segments) do not wait for their wave's worst ray
// every segment.  Four waves per SIMD (a budget of 128 VGPRs, which the shading code's peak fills:
// the radiance instances take 126-128 VGPRs and no scratch, 36 B when counting, the FULL ones
// 160-196 B of scratch; profiles/r09_wavefront_split.txt); five were measured no faster (DESIGN.md
// §3.5).
template <bool COUNT, bool FULL, bool TEAM>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(4, 4)))
wf_finish_step(DevScene S, const FrameParams* __restrict__ Pp, WfParams Q, int cur, int ts) {
    const FrameParams& P = *Pp;   // per-frame parameters in device memory
    if (cur < 0) cur = (int)__builtin_amdgcn_readfirstlane(Q.W.counts[cslot(kCntFinishQ)]);   // dev_ctl
    __shared__ int lds_stack[kStackSize * kBlock];
    __shared__ HaltonDim lds_halton[kHaltonLds];
    __shared__ MatRec lds_mat[kMatLds];
    __shared__ float4 lds_inst[3 * kInstLds];
    __shared__ Light lds_light[kLightLds];
    __shared__ float lds_sray[6][kBlock];   // each lane's shadow ray (origin, direction)
    __shared__ float lds_tx[4][kBlock];     // team drain: each leader's shadow tmax and contribution
    int* stack = &lds_stack[threadIdx.x];
    __shared__ uint32_t ts_done;
    if (threadIdx.x == 0) ts_done = 0u;
    ts_start(Q, ts);
    // (no staged spot_cone here: the second path tipped this kernel's scalar registers into spill slots)
    const ShadeTabs halton = load_tabs(S, lds_halton, lds_mat, lds_inst, lds_light, nullptr, P.U.lightCount);   // ends with a block barrier
    const Uniforms& U = P.U;
    const QueueShards qs = load_queue(Q.W.counts, cur, Q.seg_cap);   // front parts first: the likely-long paths
    const uint32_t n = queue_len(qs);
    if (Q.dev_ctl) stat_add(Q, kStatFinish, 1u);
    if (Q.dev_ctl && n > 0) stat_add(Q, kStatRounds, 1u);
    const float4* qin = Q.W.q[cur];
    const uint32_t kChunk = (uint32_t)Q.fchunk;   // paths per grab
    constexpr int kIdle = 0, kClosest = 1, kShadow = 2, kReady = 3;
    TraceCounters tc{0, 0, 0};
    bool overflow = false;
    uint32_t n_closest = 0, n_shadow = 0;
    uint32_t n_dark = 0;   // per lane (path_step runs under divergence): shadow rays with a ±0 contribution
    f2 zero2;
    zero2.x = 0.0f;
    zero2.y = 0.0f;
    uint32_t wnext = 0, wend = 0;
    bool exhausted = false;
    int mode = kIdle;
    // path
    uint32_t pid = 0;
    uint4 meta = make_uint4(0, 0, 0, 0);
    PathRegs p;
    p.color = p.accum = mk3(0, 0, 0);
    p.bounce = p.tpass = p.step = 0;
    f3 rayO = mk3(0, 0, 0), rayD = mk3(0, 0, 0), contrib = mk3(0, 0, 0);
    bool next = false;
    Trav T;
    trav_start(T, mk3(0, 0, 0), mk3(1, 0, 0), 0.0f);
    // diagnostics (Q.diag, RT_WF_LOG): segments of the longest path, loop iterations and wall
    // time (s_memrealtime, 100 MHz) of the slowest wave, time in shading passes
    uint32_t segs = 0, max_segs = 0, iters = 0;
    const uint64_t t_start = Q.diag ? __builtin_amdgcn_s_memrealtime() : 0;
    // per wave, in LDS (no registers outside RT_WF_LOG runs): iterations and ticks at its queue's
    // exhaustion, active lanes summed over the iterations after it
    __shared__ uint32_t diag_x[kBlock / 64][3];
#define RT_DX diag_x[__builtin_amdgcn_readfirstlane(threadIdx.x) / 64u]
    if (Q.diag && lane_id() == 0) RT_DX[0] = RT_DX[1] = RT_DX[2] = 0xffffffffu;
    uint64_t t_shade = 0;
    uint32_t n_pass = 0, n_shaded = 0;
    auto end_path = [&]() {
        Q.W.p_accum[pid] = make_float4(p.accum.x, p.accum.y, p.accum.z, 0.0f);
        if (Q.diag > 1) {   // RT_WF_LOG=2: segments by entry class: bounce at entry, refracting (tpass > 0) or not
            const uint32_t b0 = min(meta.z & 0xffu, (uint32_t)kDiagLenBounces - 1u), tp0 = (meta.z >> 8) & 0xffu;
            atomicAdd(&Q.W.counts[kWfDiagLen + ((tp0 ? (uint32_t)kDiagLenBounces : 0u) + b0) * (uint32_t)kDiagLenBins +
                                  min(segs, (uint32_t)kDiagLenBins - 1u)], 1u);
        }
        mode = kIdle;
        max_segs = max(max_segs, segs);
        segs = 0;
    };

    // shade this lane's closest hit (:324-774); rayO / rayD become the next ray
    auto shade_hit = [&](StepResult& r) {
        Hit h;
        h.t = T.best;
        h.id = T.best_id;
        h.u = T.bu / T.bdet;
        h.v = T.bv / T.bdet;
        const int sample = (int)meta.y;
        shade_step<FULL, false>(S, U, halton, (int)meta.w, sample, rayO, rayD, h, p, sample == 0 && p.step == 0, zero2,
                                false, zero2, r);
        write_pixel_outputs(P, meta.x, r, h, FULL);
        next = r.next;
    };
    // a lane's shadow ray in LDS: six registers fewer across the shading code
    auto sray_store = [&](f3 o, f3 d) {
        lds_sray[0][threadIdx.x] = o.x;
        lds_sray[1][threadIdx.x] = o.y;
        lds_sray[2][threadIdx.x] = o.z;
        lds_sray[3][threadIdx.x] = d.x;
        lds_sray[4][threadIdx.x] = d.y;
        lds_sray[5][threadIdx.x] = d.z;
    };
    auto sray_load = [&](uint32_t slot, f3& o, f3& d) {
        o = mk3(lds_sray[0][slot], lds_sray[1][slot], lds_sray[2][slot]);
        d = mk3(lds_sray[3][slot], lds_sray[4][slot], lds_sray[5][slot]);
    };

    // How a path advances is written once, for the three places it happens: the main loop, the lanes
    // still waiting when the team drain begins, and the drain's leaders.  They differ in:
    struct StepAt {
        bool start_next;   // the lane starts its next closest-hit query itself (trav_start); before and in
                           // the drain the team's start does it for every member, from the leader's ray
        bool in_regs;      // a shadow ray's contribution waits in `contrib` and its tmax in T.best (set by
                           // trav_start, which the loop needs anyway and the hand-over to the leaders
                           // reads); in the drain both wait in the leader's lds_tx slot
        bool fresh;        // a new query sets `fresh`: the leader's team starts it in its next iteration
    };
    constexpr StepAt kInLoop = {true, true, false}, kBeforeDrain = {false, true, false}, kInDrain = {false, false, true};
    bool fresh = false;
    auto next_query = [&](const StepAt at) {   // the path's next ray (rayO, rayD)
        if (at.start_next) trav_start(T, rayO, rayD, INFINITY);
        mode = kClosest;
        n_closest++;
        segs++;
        if (at.fresh) fresh = true;
    };
    // this lane's query ended (any: the shadow ray's, occluded or not; else the closest-hit one's)
    auto query_ended = [&](const StepAt at, bool any, bool occluded) {
        if (any) {   // unoccluded -> add its contribution (:741-743)
            if (!occluded)
                p.accum = p.accum + (at.in_regs ? contrib
                                                : mk3(lds_tx[1][threadIdx.x], lds_tx[2][threadIdx.x], lds_tx[3][threadIdx.x]));
            if (next) next_query(at);
            else end_path();
        } else if (T.best_id == 0xffffffffu) {   // miss -> path ends (:321-322)
            end_path();
        } else {
            mode = kReady;
        }
    };
    // this lane's hit is shaded: its path goes on with the shadow ray, with the next ray, or ends
    auto path_step = [&](const StepAt at) {
        StepResult r;
        shade_hit(r);
        if (r.dark) {   // counted, not traced: no query, no kShadow mode; the path goes on as after an occluded one
            n_shadow++;
            n_dark++;
        }
        if (r.shadow) {
            if (at.in_regs) {
                contrib = r.contrib;
                trav_start(T, r.so, r.sd, r.stmax);
            } else {
                lds_tx[0][threadIdx.x] = r.stmax;
                lds_tx[1][threadIdx.x] = r.contrib.x;
                lds_tx[2][threadIdx.x] = r.contrib.y;
                lds_tx[3][threadIdx.x] = r.contrib.z;
            }
            sray_store(r.so, r.sd);
            mode = kShadow;
            n_shadow++;
            if (at.fresh) fresh = true;
        } else if (r.next) {
            next_query(at);
        } else {
            end_path();
        }
    };

    while (true) {
        // ---- refill idle lanes with the next remaining paths (chunks of Q.fchunk from the XCD's counter)
        const unsigned long long idle = __ballot(mode == kIdle);
        const bool refill = __popcll(idle) >= Q.refill_min || idle == ~0ull;
        if (wnext >= wend && !exhausted && refill) {
            uint32_t base = 0;
            // this XCD's next chunk (the grid has >= 8 blocks: launch_finish)
            if (lane_id() == 0) base = atomicAdd(Q.W.counts + cslot(kCntChunkFinish + (int)(blockIdx.x & 7u)), 1u);
            base = ((__builtin_amdgcn_readfirstlane(base) << 3) | (blockIdx.x & 7u)) * kChunk;
            if (base >= n) {
                exhausted = true;
                if (Q.diag && lane_id() == 0) {
                    RT_DX[0] = iters;
                    RT_DX[1] = (uint32_t)(__builtin_amdgcn_s_memrealtime() - t_start);
                    RT_DX[2] = 0;
                }
            } else {
                wnext = base;
                wend = min(base + kChunk, n);
            }
        }
        if (idle != 0ull && wnext < wend && refill) {
            if (mode == kIdle) {
                const uint32_t g = wnext + mbcnt64(idle);
                if (g < wend) {
                    const uint32_t e = dense_entry(qs, g, Q.seg_cap);
                    const float4* src = qin + 2 * (size_t)e;
                    const float4 o = ld_stream(&src[0]);
                    const float4 d = ld_stream(&src[1]);
                    load_path(P, Q, o, d, [&]() { return ld_stream(&Q.W.qc[cur][e]); }, true, pid, meta, p);
                    rayO = ld3(o);
                    rayD = ld3(d);
                    trav_start(T, rayO, rayD, INFINITY);   // the entry's root word (qr) is not read: no register for it here
                    mode = kClosest;
                    n_closest++;
                    segs++;
                }
            }
            wnext += (uint32_t)__popcll(idle);
        }
        const unsigned long long active = __ballot(mode != kIdle);
        if (active == 0ull) break;   // idle everywhere => refill found nothing
        if (TEAM && exhausted && __popcll(active) * Q.team <= 64) break;   // the rest: team drain below
        ++iters;
        if (Q.diag && exhausted && lane_id() == 0) RT_DX[2] += (uint32_t)__popcll(active);

        // ---- one traversal step (closest hit or shadow any-hit)
        if (mode == kClosest || mode == kShadow) {
            const bool any = mode == kShadow;
            if (trav_step<COUNT>(S, T, any, stack, tc, overflow, T.best)) {
                query_ended(kInLoop, any, T.hit_any);
            }
        }

        // ---- shade the waiting lanes together (:324-774)
        const unsigned long long ready = __ballot(mode == kReady);
        int shade_thr = exhausted ? Q.shade_min_x : Q.shade_min;
        if (shade_thr < 0) shade_thr = max(1, -shade_thr * __popcll(__ballot(mode != kIdle)) / 100);   // % of the busy lanes
        if (ready != 0ull && (__popcll(ready) >= shade_thr || __ballot(mode == kClosest || mode == kShadow) == 0ull)) {
            const uint64_t ts0 = Q.diag ? __builtin_amdgcn_s_memrealtime() : 0;
            if (Q.diag) {
                ++n_pass;
                n_shaded += (uint32_t)__popcll(ready);
            }
            if (mode == kReady) path_step(kInLoop);
            // Every lane's ray setup is rebuilt from its ray (a pure function of it, so bit for bit
            // the one trav_start made): the ~19 registers of the traversing lanes' setups are then
            // dead while the shading code runs, which sets the kernel's register peak.
            if (mode == kShadow) {
                f3 so, sd;
                sray_load(threadIdx.x, so, sd);
                T.R = ray_setup(so, sd);
            } else {
                T.R = ray_setup(rayO, rayD);
            }
            if (Q.diag) t_shade += __builtin_amdgcn_s_memrealtime() - ts0;
        }

    }

    // ---- team drain (Q.team lanes per query).  The queue has run out and this wave holds at most
    // 64 / team paths: each moves to a team leader (lane team * r) and the team's lanes traverse its
    // query together, splitting the node groups and stack entries among themselves (XOR-paired
    // hand-offs every iteration) and sharing the closest hit found so far as their cull bound; a
    // closest-hit query ends with the lexicographic minimum of the members' (t, id), the serial
    // traversal's result, so the same bits; an any-hit query ends at any member's occluder.  The
    // leader shades, then the team starts the path's next query.
    if (TEAM && __ballot(mode != kIdle) != 0ull) {
        const int TM = Q.team;
        if (mode == kReady) path_step(kBeforeDrain);   // waiting lanes first: every busy lane then holds a query
        const unsigned long long busy = __ballot(mode != kIdle);
        const int lane = (int)lane_id(), j = lane & (TM - 1), lead = lane - j, rk = lane / TM;
        const int nb = __popcll(busy);
        int src = lane;   // team leader rk takes the rk-th busy lane's path
        {
            unsigned long long b = busy;
            for (int k = 0; b; ++k) {
                const int l = __builtin_ctzll(b);
                b &= b - 1ull;
                if (j == 0 && rk == k) src = l;
            }
        }
        const bool leader = j == 0 && rk < nb;
        auto mvu = [&](uint32_t v) { return (uint32_t)__shfl((int)v, src); };
        auto mvf = [&](float v) { return __shfl(v, src); };
        auto mv3 = [&](f3 v) { return mk3(mvf(v.x), mvf(v.y), mvf(v.z)); };
        const uint32_t sbase = threadIdx.x & ~63u;
        // the leaders' shadow rays stay in LDS (each leader's slot; the members read it when the
        // team starts the query)
        {
            f3 so, sd;
            sray_load(sbase + (uint32_t)src, so, sd);
            sray_store(so, sd);
        }
        // the leaders' shadow tmax and contribution stay in LDS as well (lds_tx)
        {
            const float t_src = mvf(T.best);
            const f3 c_src = mv3(contrib);
            lds_tx[0][threadIdx.x] = t_src;
            lds_tx[1][threadIdx.x] = c_src.x;
            lds_tx[2][threadIdx.x] = c_src.y;
            lds_tx[3][threadIdx.x] = c_src.z;
        }
        pid = mvu(pid);
        meta = make_uint4(mvu(meta.x), mvu(meta.y), mvu(meta.z), mvu(meta.w));
        p.color = mv3(p.color);
        p.accum = mv3(p.accum);
        p.bounce = (int)mvu((uint32_t)p.bounce);
        p.step = (int)mvu((uint32_t)p.step);
        p.tpass = (int)mvu((uint32_t)p.tpass);
        rayO = mv3(rayO);
        rayD = mv3(rayD);
        next = mvu(next ? 1u : 0u) != 0u;
        segs = mvu(segs);
        // every lane takes part in the shuffle: a bpermute inside the leaders' branch would read the
        // (inactive) non-leader source lanes as zero
        const int src_mode = (int)mvu((uint32_t)mode);
        mode = leader ? src_mode : kIdle;
        fresh = leader;   // the team starts the leader's query
        float cull = INFINITY;
        while (true) {
            const int lmode = __shfl(mode, lead);
            if (__ballot(lmode != kIdle) == 0ull) break;
            const bool team_on = lmode == kClosest || lmode == kShadow, any = lmode == kShadow;
            if (__shfl((int)fresh, lead) != 0 && team_on) {   // start the team's query on every member
                f3 o, d;
                float tmax;
                if (any) {
                    const uint32_t ls = sbase + (uint32_t)lead;
                    sray_load(ls, o, d);
                    tmax = lds_tx[0][ls];
                } else {
                    o = mk3(__shfl(rayO.x, lead), __shfl(rayO.y, lead), __shfl(rayO.z, lead));
                    d = mk3(__shfl(rayD.x, lead), __shfl(rayD.y, lead), __shfl(rayD.z, lead));
                    tmax = INFINITY;
                }
                trav_start(T, o, d, tmax);
                if (j != 0) T.g_hits = 0;   // members start without work; the leader hands it out below
                cull = tmax;
            }
            fresh = false;
            // one traversal step of every member with work
            if (team_on && !(T.t_mask == 0u && T.g_hits == 0u && T.sp == 0))
                (void)trav_step<COUNT>(S, T, any, stack, tc, overflow, cull);
            // occluder anywhere in the team; the team's closest hit so far (the cull bound)
            int hit = (any && T.hit_any) ? 1 : 0;
            float bt = T.best;
            for (int k = 1; k < TM; k <<= 1) {
                hit |= __shfl_xor(hit, k);
                bt = fminf(bt, __shfl_xor(bt, k));
            }
            if (team_on && !any) cull = bt;
            if (hit) {
                T.t_mask = 0u;
                T.g_hits = 0u;
                T.sp = 0;
            }
            // hand-offs: in round k lane l pairs with lane l ^ k; an idle member takes the later
            // half (in visiting order) of its partner's node group, or its partner's top stack entry
            for (int k = 1; k < TM; ++k) {
                const bool idle_m = team_on && T.t_mask == 0u && T.g_hits == 0u && T.sp == 0;
                const bool give = team_on && (__popc(T.g_hits) >= 2 || T.sp > 0);
                const bool p_idle = __shfl_xor((int)idle_m, k) != 0, p_give = __shfl_xor((int)give, k) != 0;
                uint32_t pay = 0u;
                if (give && p_idle) {
                    if (__popc(T.g_hits) >= 2) {
                        uint32_t keep = 0u, rest = T.g_hits;
                        for (int c = __popc(T.g_hits) - __popc(T.g_hits) / 2; c > 0; --c) {
                            const int b = T.g_flip ? highest_bit(rest) : lowest_bit(rest);
                            keep |= 1u << b;
                            rest &= ~(1u << b);
                        }
                        pay = pack_group(T.g_base, T.g_flip, rest);
                        T.g_hits = keep;
                    } else {
                        --T.sp;
                        pay = (uint32_t)stack[T.sp * kBlock];
                    }
                }
                const uint32_t got = (uint32_t)__shfl_xor((int)pay, k);
                if (idle_m && p_give) {
                    unpack_group(got, T.g_base, T.g_flip, T.g_hits);
                }
            }
            // the team's query has ended once no member holds work
            int work = (team_on && !(T.t_mask == 0u && T.g_hits == 0u && T.sp == 0)) ? 1 : 0;
            for (int k = 1; k < TM; k <<= 1) work |= __shfl_xor(work, k);
            if (team_on && !work) {
                if (!any) {   // lexicographic minimum of the members' (t, id), with its (V, W, det)
                    float t = T.best, bu = T.bu, bv = T.bv, bd = T.bdet;
                    uint32_t id = T.best_id;
                    for (int k = 1; k < TM; k <<= 1) {
                        const float t2 = __shfl_xor(t, k), u2 = __shfl_xor(bu, k), v2 = __shfl_xor(bv, k),
                                    d2 = __shfl_xor(bd, k);
                        const uint32_t id2 = (uint32_t)__shfl_xor((int)id, k);
                        if (t2 < t || (t2 == t && id2 < id)) {
                            t = t2;
                            id = id2;
                            bu = u2;
                            bv = v2;
                            bd = d2;
                        }
                    }
                    T.best = t;
                    T.best_id = id;
                    T.bu = bu;
                    T.bv = bv;
                    T.bdet = bd;
                }
                if (j == 0) query_ended(kInDrain, any, hit != 0);   // the leader: the path's next step
            }
            if (mode == kReady) path_step(kInDrain);   // leaders: shade at once (the drain is latency-bound)
        }
    }

    if (Q.diag) {
        const uint32_t dt = (uint32_t)(__builtin_amdgcn_s_memrealtime() - t_start);
        if (lane_id() == 0) {
            const uint32_t* dx = RT_DX;
            const bool x = dx[0] != 0xffffffffu;   // else its last grab was in range: it never saw the end
            const uint32_t it_x = x ? dx[0] : iters, t_x = x ? dx[1] : dt;
            atomicAdd(&Q.W.counts[kWfStat + kStatDiagItPre], it_x);
            atomicAdd(&Q.W.counts[kWfStat + kStatDiagItPost], iters - it_x);
            atomicAdd(&Q.W.counts[kWfStat + kStatDiagTPre], t_x);
            atomicAdd(&Q.W.counts[kWfStat + kStatDiagTPost], dt - t_x);
            atomicAdd(&Q.W.counts[kWfStat + kStatDiagLanesPost], x ? dx[2] : 0u);
            atomicAdd(&Q.W.counts[kWfDiagExh + min(t_x / kDiagTimeBinTicks, (uint32_t)kDiagTimeBins - 1u)], 1u);
            atomicAdd(&Q.W.counts[kWfStat + kStatDiagShadeT], (uint32_t)t_shade);
            atomicAdd(&Q.W.counts[kWfStat + kStatDiagTotalT], dt);
            atomicAdd(&Q.W.counts[kWfStat + kStatDiagPasses], n_pass);
            atomicAdd(&Q.W.counts[kWfStat + kStatDiagShaded], n_shaded);
        }
        for (int off = 32; off > 0; off >>= 1) max_segs = max(max_segs, (uint32_t)__shfl_xor((int)max_segs, off, 64));
        if (lane_id() == 0) {
            atomicMax(&Q.W.counts[cslot(kCntDiagSegs)], max_segs);
            atomicMax(&Q.W.counts[cslot(kCntDiagIters)], iters);
            atomicMax(&Q.W.counts[cslot(kCntDiagTime)], dt);
            atomicAdd(&Q.W.counts[kWfDiagHist + min(dt / kDiagTimeBinTicks, (uint32_t)kDiagTimeBins - 1u)], 1u);
        }
    }
#undef RT_DX
    ts_end(Q, ts, &ts_done);
    flush_counters<true>(P, n_closest, n_shadow, 0, tc, COUNT, overflow, false, 0u, n_dark);
}

// ---- motion-adaptive extra samples (:779-789) -----------------------------------------------------------
__global__ void __launch_bounds__(kBlock) wf_extra(DevScene S, const FrameParams* __restrict__ Pp, WfParams Q, int qidx) {
    const FrameParams& P = *Pp;   // per-frame parameters in device memory
    __shared__ HaltonDim lds_halton[kHaltonLds];
    const ShadeTabs halton = load_tabs(S, lds_halton, nullptr);   // no shading: Halton only
    const Uniforms& U = P.U;
    const int maxExtra = (U.enableMotionAdaptiveSampling != 0) ? max(U.motionSamplingMaxExtraSamples, 0) : 0;
    const int stride = Q.spp + maxExtra;
    const int shard = blockIdx.x & (kShards - 1);
    float4* qout = Q.W.q[qidx] + 2 * (size_t)shard * Q.seg_cap;
    uint32_t* qrout = Q.W.qr[qidx] + (size_t)shard * Q.seg_cap;
    __shared__ BlockAlloc ba;
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    int px = 0, py = 0, e = 0;
    uint32_t pix = 0;
    if (i < Q.own_pixels) {
        own_pixel(Q.px, i, px, py);
        if (px < U.width && py < U.height) {
            pix = (uint32_t)py * (uint32_t)U.width + (uint32_t)px;
            float2 mv2 = P.motion[pix], pm2 = P.motion_prev[pix];
            f2 mv, pm;
            mv.x = mv2.x;
            mv.y = mv2.y;
            pm.x = pm2.x;
            pm.y = pm2.y;
            e = extra_samples(U, maxExtra, mv, pm);
        }
    }
    const uint32_t start = block_alloc_n((uint32_t)e, &Q.W.counts[cslot(kCntExtra)], ba);
    const uint32_t slot0 =
        block_alloc_n(U.maxBounces > 0 ? (uint32_t)e : 0u, &Q.W.counts[cslot(qidx * kShards + shard)], ba);
    if (e > 0) {
        const uint32_t offset = P.random[pix];
        for (int j = 0; j < e; ++j) {
            int s = Q.spp + j;
            uint32_t pid = Q.base_paths + start + (uint32_t)j;
            int hidx = (int)(offset + (unsigned)((int)U.frameIndex * stride + s));
            init_path(Q, pid, pix, s, (uint32_t)hidx);
            f3 o, d;
            primary_ray(U, halton, px, py, hidx, o, d);
            if (U.maxBounces > 0) {
                const uint32_t slot = slot0 + (uint32_t)j;
                qout[2 * (size_t)slot] = make_float4(o.x, o.y, o.z, __uint_as_float(pid));
                qout[2 * (size_t)slot + 1] = make_float4(d.x, d.y, d.z, 0.0f);
                qrout[slot] = 0u;   // no root word: extend tests the root itself (few rays, and not every frame)
            }
        }
    }
    if (i < Q.own_pixels) Q.W.px_extra[i] = make_uint2(start, (uint32_t)e);
    TraceCounters tc{0, 0, 0};
    flush_counters(P, 0, 0, (uint32_t)e, tc, false, false);
}

// ---- depth + motion (:342-389) ----------------------------------------------------------------------
// After the base pass: every own pixel whose sample 0 had a bounce-0 hit gets the depth and motion
// vector of the last such hit (the value the per-pixel kernel leaves, since each of those hits
// overwrites it), evaluated here once instead of inside every shading launch, where it would
// hold ~25 VGPRs of transforms and cameras.
__global__ void __launch_bounds__(kBlock) wf_motion(DevScene S, const FrameParams* __restrict__ Pp, WfParams Q) {
    const FrameParams& P = *Pp;
    const Uniforms& U = P.U;
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= Q.own_pixels) return;
    int px, py;
    own_pixel(Q.px, i, px, py);
    if (px >= U.width || py >= U.height) return;
    const size_t pix = (size_t)py * U.width + px;
    const uint4 ph = P.prim_hit[pix];
    if (ph.x == 0xffffffffu) return;   // no bounce-0 hit: generate's defaults stay
    float depth;
    f2 mv;
    primary_outputs(S, U, ph.x, __uint_as_float(ph.y), __uint_as_float(ph.z), depth, mv);
    P.depth[pix] = depth;
    P.motion[pix] = make_float2(mv.x, mv.y);
}

// ---- resolve (:777, :792-819) -------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock) wf_resolve(DevScene S, const FrameParams* __restrict__ Pp, WfParams Q, int with_extra) {
    const FrameParams& P = *Pp;   // per-frame parameters in device memory
    const Uniforms& U = P.U;
    uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= Q.own_pixels) return;
    int px, py;
    own_pixel(Q.px, i, px, py);
    if (px >= U.width || py >= U.height) return;
    size_t pix = (size_t)py * U.width + px;
    f3 total = mk3(0.0f, 0.0f, 0.0f);
    for (int s = 0; s < Q.spp; ++s) {
        float4 a = Q.W.p_accum[(size_t)i * Q.spp + s];
        total = total + mk3(a.x, a.y, a.z);
    }
    int nsamp = Q.spp;
    if (with_extra) {
        uint2 ex = Q.W.px_extra[i];
        for (uint32_t j = 0; j < ex.y; ++j) {
            float4 a = Q.W.p_accum[Q.base_paths + ex.x + j];
            total = total + mk3(a.x, a.y, a.z);
        }
        nsamp += (int)ex.y;
    }
    float2 mv2 = P.motion[pix], pm2 = P.motion_prev[pix];
    f2 mv, pm;
    mv.x = mv2.x;
    mv.y = mv2.y;
    pm.x = pm2.x;
    pm.y = pm2.y;
    f3 c = resolve_pixel(U, total, nsamp, mv, pm, P.accum_in, pix);
    P.accum_out[pix] = make_float4(c.x, c.y, c.z, 1.0f);
}

// ---- the kernel instances, handed to the scheduler (rt_wavefront_host.cpp) ---------------------------
// resident blocks (CUs x blocks per CU) of a persistent kernel
template <typename K>
static unsigned resident_grid(K kernel, int fallback_per_cu) {
    int dev = 0, cus = 256, per = 0;
    if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, kernel, kBlock, 0) != hipSuccess || per < 1)
        per = fallback_per_cu;
    return (unsigned)(cus * per);
}

template <bool COUNT, bool FULL, bool SORTED, bool TEAM>
static WfKernels kernel_set() {
    WfKernels K = {wf_trace<false, COUNT>, wf_trace<true, COUNT>, wf_finish_step<COUNT, FULL, TEAM>,   // extend, connect, finish
                   wf_shade<FULL, SORTED>, wf_extra, wf_resolve, wf_generate, wf_motion,
                   wf_sort_hist, wf_sort_scatter, wf_sort_rowscan, 0u, 0u};
    // the team instance is sized by its own occupancy (its LDS and registers differ)
    K.finish_resident = resident_grid(K.finish, 2);
    return K;
}

template <size_t... I>
static std::array<WfKernels, 16> kernel_table(std::index_sequence<I...>) {
    std::array<WfKernels, 16> t = {{kernel_set<(I >> 3) & 1, (I >> 2) & 1, (I >> 1) & 1, I & 1>()...}};
    const unsigned trace = resident_grid(t[0].extend, 4);   // every traversal launch is sized by the plain extend instance
    for (WfKernels& k : t) k.trace_resident = trace;
    return t;
}

const WfKernels& wf_kernels(bool count, bool full, bool sorted, bool team) {
    static const std::array<WfKernels, 16> table = kernel_table(std::make_index_sequence<16>());
    return table[(count ? 8 : 0) | (full ? 4 : 0) | (sorted ? 2 : 0) | (team ? 1 : 0)];
}

}  // namespace rt

