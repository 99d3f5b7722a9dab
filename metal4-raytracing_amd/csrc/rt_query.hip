// rt_query.hip — device ray queries (rt_trace_closest / rt_trace_any, include/rt_api.h): the
// caller's rays traced against the built scene by one persistent launch, built from the stepwise
// traversal of rt_trav.h the way wf_trace (rt_wavefront.hip) is.  The replacement of Metal's
// `intersector.intersect` called from a kernel other than raytracingKernel.  Next to it the two
// per-record kernels of a user-side integrator: rq_resolve (rt_resolve_hits) and rq_shade
// (rt_shade_hits).
#include <hip/hip_runtime.h>

#include "rt_kernels.h"
#include "rt_scatter.h"
#include "rt_surface.h"
#include "rt_trav.h"
#include "rt_wf_queue.h"   // lane_id, mbcnt64

namespace rt {

namespace {

constexpr uint32_t kMiss = 0xffffffffu;
constexpr uint32_t kChunkCtrStride = 32;   // 32-bit words per chunk counter: one 128-B line each

// ---- persistent traversal of a flat ray array with per-lane refill ------------------------------------
// The grid is at most the resident capacity.  The array is cut into chunks of kRqChunk consecutive
// rays; chunk c belongs to counter c % 8, and XCD k (blockIdx % 8) hands out the chunks of counter
// k, one atomic per chunk, then those of the next counter once its own have run out (so any grid,
// a single block included, covers every ray, and an XCD that finishes early helps the others).
// Every iteration advances each lane one trav_step; idle lanes take the next rays of the wave's
// chunk once Q.refill_min lanes are idle, so a refilling wave reads consecutive 32-B records.
// A lane whose query ends writes its record: closest hit two 16-B words (the second one behind two
// dependent lookups: tri_info[id].w, then the submesh's first triangle), any hit one word.
template <bool ANY, bool COUNT>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(8, 8)))
rq_trace(DevScene S, RqParams Q) {
    __shared__ int lds_stack[kStackSize * kBlock];
    int* stack = &lds_stack[threadIdx.x];

    uint32_t* const chunk_ctr = reinterpret_cast<uint32_t*>(Q.state + kCounterWords);
    const uint32_t nchunks = (Q.n - 1u) / (uint32_t)kRqChunk + 1u;   // n > 0
    const uint32_t xcd = blockIdx.x & (uint32_t)(kRqChunkCounters - 1);
    uint32_t tries = 0;   // counters found exhausted so far (wave-uniform)
    uint32_t wnext = 0, wend = 0;

    TraceCounters tc{0, 0, 0};
    bool overflow = false;
    uint32_t rays = 0, nhit = 0;
    bool active = false;
    uint32_t idx = 0;
    Trav T;
    trav_start(T, mk3(0, 0, 0), mk3(1, 0, 0), 0.0f);

    while (true) {
        // refill idle lanes from the wave's chunk
        const unsigned long long idle = __ballot(!active);
        const bool refill = __popcll(idle) >= Q.refill_min || idle == ~0ull;
        if (refill) {
            while (wnext >= wend && tries < (uint32_t)kRqChunkCounters) {
                const uint32_t part = (xcd + tries) & (uint32_t)(kRqChunkCounters - 1);
                uint32_t k = 0;
                if (lane_id() == 0) k = atomicAdd(&chunk_ctr[part * kChunkCtrStride], 1u);
                k = __builtin_amdgcn_readfirstlane(k);
                // chunk k of counter `part`: k stays below nchunks / 8 + the waves of the grid, far from 2^29
                const uint32_t c = k * (uint32_t)kRqChunkCounters + part;
                if (c >= nchunks) {
                    ++tries;
                } else {
                    wnext = c * (uint32_t)kRqChunk;   // < n
                    wend = Q.n - wnext < (uint32_t)kRqChunk ? Q.n : wnext + (uint32_t)kRqChunk;
                }
            }
        }
        if (idle != 0ull && wnext < wend && refill) {
            if (!active) {
                const uint32_t g = wnext + mbcnt64(idle);
                if (g < wend) {
                    const float4 o4 = Q.rays[2 * (size_t)g];
                    const float4 d4 = Q.rays[2 * (size_t)g + 1];
                    trav_start(T, ld3(o4), ld3(d4), d4.w);
                    active = true;
                    idx = g;
                    rays++;
                }
            }
            wnext = min(wnext + (uint32_t)__popcll(idle), wend);
        }
        if (__ballot(active) == 0ull) break;   // nothing left: every counter has run out
        if (active && trav_step<COUNT>(S, T, ANY, stack, tc, overflow, T.best)) {
            active = false;
            if (ANY) {
                Q.occluded[idx] = T.hit_any ? 1u : 0u;
                nhit += T.hit_any ? 1u : 0u;
            } else {
                const bool hit = T.best_id != kMiss;
                float4 w0 = make_float4(INFINITY, 0.0f, 0.0f, __uint_as_float(kMiss));
                uint4 w1 = make_uint4(kMiss, kMiss, kMiss, 0u);
                if (hit) {
                    w0 = make_float4(T.best, T.bu / T.bdet, T.bv / T.bdet, __uint_as_float(T.best_id));
                    const uint32_t w = S.tri_info[T.best_id].w;   // mesh << 8 | submesh
                    const uint32_t mesh = w >> 8, sub = w & 0xffu;
                    const uint32_t first = Q.sub_first[(size_t)mesh * (uint32_t)S.max_submeshes + sub];
                    w1 = make_uint4(mesh, sub, T.best_id - first, 0u);
                    nhit++;
                }
                Q.hits[2 * (size_t)idx] = w0;
                reinterpret_cast<uint4*>(Q.hits)[2 * (size_t)idx + 1] = w1;
            }
        }
    }
    block_flush_counters(Q.state, ANY ? 0u : rays, ANY ? rays : 0u, COUNT ? tc.nodes : 0u, COUNT ? tc.tris : 0u, nhit,
                         overflow);
}

// ---- surface queries: a ray and its hit record -> rt_surface (+ rt_surface_material) ---------------
// One record per thread, grid-stride over at most the resident blocks.  Per record two 16-B loads
// of the ray, two of the hit, the triangle's tri_nrm line (its fourth word only when the submesh
// has a bound map), the instance matrix and the Material straight from global memory (KBs, cache
// resident: staging them in LDS per block would cost small batches more than it saves), then four
// 16-B stores, seven with materials.  No LDS, no atomics.  The record index stays 64-bit: n may
// be anything below 2^32 and the last stride may step past it.
template <bool MATERIAL, bool TEXTURED>
__global__ void __launch_bounds__(kBlock) rq_resolve(DevScene S, RsParams P) {
    const size_t stride = (size_t)gridDim.x * kBlock;
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < (size_t)P.n; i += stride) {
        const float4 o4 = P.rays[2 * i], d4 = P.rays[2 * i + 1];
        const float4 h0 = P.hits[2 * i];
        const uint4 h1 = reinterpret_cast<const uint4*>(P.hits)[2 * i + 1];
        SurfaceWords r;
        surface_eval<MATERIAL, TEXTURED>(S, o4, d4, h0, h1, r);
        float4* const so = P.surfaces + 4 * i;
        so[0] = r.s0;
        so[1] = r.s1;
        so[2] = r.s2;
        reinterpret_cast<uint4*>(so)[3] = r.s3;
        if (MATERIAL) {
            float4* const mo = P.materials + 3 * i;
            mo[0] = r.m0;
            mo[1] = r.m1;
            mo[2] = r.m2;
        }
    }
}

// ---- shading queries: a resolved hit and its path state -> the path's next rays ---------------------
// One record per thread, grid-stride over at most the resident blocks, as rq_resolve.  Per record
// eleven 16-B loads (the ray's direction word, four of the surface, three of the material, three
// of the path; two more with the caller's numbers) and eight 16-B stores (path, next ray, shadow
// ray, contribution).  The Halton dimensions and the lights are read from global memory: a record
// draws at most four dimensions (16 B each) chosen by its own step, glass paths reach dimensions
// past the 64 an LDS copy would hold, and the whole table is 16 KB, cache resident after the first
// wave; staging tables per block would cost small batches more than it saves (rq_resolve's choice).
// No LDS, no atomics.  next_rays may alias rays: a thread reads its record before it writes it.
template <bool RANDOMS>
__global__ void __launch_bounds__(kBlock) rq_shade(ShParams P) {
    const ScatterOpts U{P.shading_mode, P.max_bounces, P.light_count};
    const size_t stride = (size_t)gridDim.x * kBlock;
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < (size_t)P.n; i += stride) {
        const float4 d4 = P.rays[2 * i + 1];
        const float4* const sp = P.surfaces + 4 * i;
        const float4 s0 = sp[0], s1 = sp[1], s2 = sp[2];
        const uint4 s3 = reinterpret_cast<const uint4*>(sp)[3];
        const float4* const mp = P.materials + 3 * i;
        const float4 m0 = mp[0], m1 = mp[1], m2 = mp[2];
        float4* const pp = P.paths + 3 * i;
        PathWords w;
        w.p0 = pp[0];
        w.p1 = pp[1];
        w.p2 = reinterpret_cast<const int4*>(pp)[2];
        float4 r0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), r1 = r0;
        if (RANDOMS) {
            r0 = P.randoms[2 * i];
            r1 = P.randoms[2 * i + 1];
        }
        ScatterOut o;
        scatter_eval<RANDOMS>(P.halton, P.lights, U, d4, s0, s1, s2, s3, m0, m1, m2, r0, r1, w, o);
        pp[0] = w.p0;
        pp[1] = w.p1;
        reinterpret_cast<int4*>(pp)[2] = w.p2;
        P.next_rays[2 * i] = o.n0;
        P.next_rays[2 * i + 1] = o.n1;
        P.shadow_rays[2 * i] = o.h0;
        P.shadow_rays[2 * i + 1] = o.h1;
        P.contrib[i] = o.c;
    }
}

}  // namespace

unsigned shade_resident_blocks() {
    static const unsigned resident = [] {
        int dev = 0, cus = 256, per = 0;
        if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, rq_shade<false>, kBlock, 0) != hipSuccess || per < 1) per = 4;
        return (unsigned)(cus * per);
    }();
    return resident;
}

void launch_shade(const ShParams& P, unsigned blocks, hipStream_t stream) {
    auto kernel = P.randoms ? rq_shade<true> : rq_shade<false>;
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kBlock), 0, stream, P);
}

unsigned resolve_resident_blocks() {
    static const unsigned resident = [] {
        int dev = 0, cus = 256, per = 0;
        if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
        // the variant that holds the most registers: one figure serves all four
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, rq_resolve<true, true>, kBlock, 0) != hipSuccess || per < 1)
            per = 4;
        return (unsigned)(cus * per);
    }();
    return resident;
}

void launch_resolve(const DevScene& S, const RsParams& P, unsigned blocks, hipStream_t stream) {
    const bool mat = P.materials != nullptr, tex = S.textured != 0;
    auto kernel = mat ? (tex ? rq_resolve<true, true> : rq_resolve<true, false>)
                      : (tex ? rq_resolve<false, true> : rq_resolve<false, false>);
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kBlock), 0, stream, S, P);
}

unsigned query_resident_blocks() {
    static const unsigned resident = [] {
        int dev = 0, cus = 256, per = 0;
        if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, rq_trace<false, false>, kBlock, 0) != hipSuccess || per < 1)
            per = 4;
        return (unsigned)(cus * per);
    }();
    return resident;
}

void launch_query(const DevScene& S, const RqParams& Q, bool any, bool count, unsigned blocks, hipStream_t stream) {
    auto kernel = any ? (count ? rq_trace<true, true> : rq_trace<true, false>)
                      : (count ? rq_trace<false, true> : rq_trace<false, false>);
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kBlock), 0, stream, S, Q);
}

}  // namespace rt
