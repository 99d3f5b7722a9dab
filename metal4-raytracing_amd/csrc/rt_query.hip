// rt_query.hip — device ray queries (rt_trace_closest / rt_trace_any, include/rt_api.h): the
// caller's rays traced against the built scene by one persistent launch, built from the stepwise
// traversal of rt_trav.h the way wf_trace (rt_wavefront.hip) is.  The replacement of Metal's
// `intersector.intersect` called from a kernel other than raytracingKernel.
#include <hip/hip_runtime.h>

#include "rt_kernels.h"
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

}  // namespace

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
