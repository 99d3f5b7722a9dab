// rt_query.hip — device ray queries (rt_trace_closest / rt_trace_any, include/rt_api.h): the
// caller's rays traced against the built scene by one persistent launch, built from the stepwise
// traversal of rt_trav.h the way wf_trace (rt_wavefront.hip) is.  The replacement of Metal's
// `intersector.intersect` called from a kernel other than raytracingKernel.  Next to it the two
// per-record kernels of a user-side integrator: rq_resolve (rt_resolve_hits) and rq_shade
// (rt_shade_hits), and the path queries that close its loop: rq_camera, rq_connect, rq_retire,
// rq_average and the three launches of rt_compact_paths.  Every kernel whose record count a
// compaction can produce reads it through launch_count (rt_kernels.h): the host's n, or for the
// _indirect entry points a device word clamped to it, so the grid needs a bound only.
#include <hip/hip_runtime.h>

#include "rt_kernels.h"
#include "rt_paths.h"
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
    const uint32_t n = launch_count(Q.count, Q.n);
    const uint32_t nchunks = (n - 1u) / (uint32_t)kRqChunk + 1u;   // n > 0: read inside the loop only
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

    // A device count of 0 (the host never launches n == 0): no wave enters, no chunk counter is
    // touched, and every wave flushes its zeros below.
    if (n != 0u) while (true) {
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
                // (a wave adds to a counter it found exhausted once, then moves on: the second term is the
                // grid's, at most the resident waves, however far a device count falls below its bound)
                const uint32_t c = k * (uint32_t)kRqChunkCounters + part;
                if (c >= nchunks) {
                    ++tries;
                } else {
                    wnext = c * (uint32_t)kRqChunk;   // < n
                    wend = n - wnext < (uint32_t)kRqChunk ? n : wnext + (uint32_t)kRqChunk;
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
    const size_t n = launch_count(P.count, P.n);
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
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
    const size_t n = launch_count(P.count, P.n);
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
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

// ---- path queries: camera paths, connect, retire, average -------------------------------------------
// One record per thread, grid-stride over at most the resident blocks, as rq_shade; every record
// moves as whole 16-B words, the per-record code is rt_paths.h's.  No LDS, no atomics.
__global__ void __launch_bounds__(kBlock) rq_camera(CamParams P) {
    const HaltonDim tab1 = P.halton[1];
    const size_t stride = (size_t)gridDim.x * kBlock;
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < (size_t)P.n; i += stride) {
        const uint32_t pix = P.first_pixel + (uint32_t)i;   // < width * height (checked by the host)
        CameraWords w;
        camera_record(P.U, tab1, P.random[pix], pix, P.sample, pix * P.tag_stride + P.tag_offset, w);
        P.rays[2 * i] = w.r0;
        P.rays[2 * i + 1] = w.r1;
        float4* const pp = P.paths + 3 * i;
        pp[0] = w.p0;
        pp[1] = w.p1;
        reinterpret_cast<uint4*>(pp)[2] = w.p2;
    }
}

// Shadow ray j (of m) belongs to record index[j] (or j); an unoccluded one adds its record's
// contribution.  Records at or above n are skipped before anything of theirs is addressed.  A
// device count bounds the shadow rays (m); n is always the host's.
__global__ void __launch_bounds__(kBlock) rq_connect(ConnectParams P) {
    const size_t stride = (size_t)gridDim.x * kBlock;
    const size_t m = launch_count(P.count, P.m);
    for (size_t j = (size_t)blockIdx.x * kBlock + threadIdx.x; j < m; j += stride) {
        if (P.occluded[j] != 0u) continue;
        const size_t i = P.index ? (size_t)P.index[j] : j;
        if (i >= (size_t)P.n) continue;
        P.paths[3 * i + 1] = connect_word(P.paths[3 * i + 1], P.contrib[i]);
    }
}

__global__ void __launch_bounds__(kBlock) rq_retire(RetireParams P) {
    const size_t stride = (size_t)gridDim.x * kBlock;
    const size_t n = launch_count(P.count, P.n);
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const float4 p1 = P.paths[3 * i + 1];
        const uint32_t tag = reinterpret_cast<const uint4*>(P.paths)[3 * i + 2].w;
        if ((f2u(p1.w) & RT_PATH_ALIVE) == 0u && tag < P.tags) P.samples[tag] = retire_word(p1);
    }
}

__global__ void __launch_bounds__(kBlock) rq_average(AverageParams P) {
    const size_t stride = (size_t)gridDim.x * kBlock;
    for (size_t p = (size_t)blockIdx.x * kBlock + threadIdx.x; p < (size_t)P.pixels; p += stride)
        P.rgba[p] = average_pixel(P.samples + p * P.spp, P.spp);
}

// ---- path queries: stable compaction ------------------------------------------------------------------
// Three launches, none of which waits for another block (no look-back, no ticket, no grid
// barrier): the order of the output is the order of the input whatever order the blocks run in.
//  1. rq_compact_count: per tile of kCompactTile records, the selection word of each 64-record
//     segment (a wave's __ballot of (flags & mask) != 0; the flag words sit 48 B apart, so this is
//     the one launch that touches every line of `paths`) and the tile's selected count.
//  2. rq_compact_scan: one block turns the tile counts into exclusive offsets, kBlock at a time
//     with a running carry, and writes *count.
//  3. rq_compact_copy: per tile, the rank of a selected record is its segment's base (an LDS scan
//     of the kCompactSegs popcounts) plus mbcnt of the segment's word below its lane; the tile's
//     selected source indices are staged in LDS in rank order, and consecutive threads then copy
//     consecutive 16-B words of the tile's contiguous destination range [offset, offset + cnt):
//     coalesced stores, gathering loads.  It reads the 8-byte words of launch 1, not the flags.
// With a device count each launch runs over the tiles of min(*n_count, n) only (none for 0: the
// scan still writes *count = 0); the scratch keeps the layout of P.tiles = compact_tiles(n).
static_assert(kCompactTile % kBlock == 0 && kBlock % 64 == 0 && kCompactSegs <= kBlock, "tile geometry");

__device__ __forceinline__ uint32_t launch_tiles(uint32_t n) { return n ? compact_tiles(n) : 0u; }   // <= P.tiles

__global__ void __launch_bounds__(kBlock) rq_compact_count(CompactParams P) {
    __shared__ uint32_t seg_cnt[kCompactSegs];
    const uint32_t wave = threadIdx.x >> 6;
    const uint32_t* const flags = reinterpret_cast<const uint32_t*>(P.paths) + 7;   // rt_path.flags, 12 words apart
    const uint32_t n = launch_count(P.n_count, P.n), tiles = launch_tiles(n);
    for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const size_t first = (size_t)tile * kCompactTile;
        #pragma unroll
        for (uint32_t k = 0; k < kCompactTile / kBlock; ++k) {
            const size_t i = first + k * kBlock + threadIdx.x;
            const bool sel = i < (size_t)n && (flags[12 * i] & P.mask) != 0u;
            const unsigned long long b = __ballot(sel);
            if (lane_id() == 0) {
                const uint32_t seg = k * (kBlock / 64) + wave;
                P.bits[(size_t)tile * kCompactSegs + seg] = b;   // segments past n: 0
                seg_cnt[seg] = (uint32_t)__popcll(b);
            }
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t s = 0;
            #pragma unroll
            for (uint32_t q = 0; q < kCompactSegs; ++q) s += seg_cnt[q];
            P.tile_count[tile] = s;
        }
        __syncthreads();   // seg_cnt is rewritten by the next tile
    }
}

// One block whatever n is.  The total is at most n, so 32 bits hold every offset and the count.
__global__ void __launch_bounds__(kBlock) rq_compact_scan(CompactParams P) {
    __shared__ uint32_t wave_tot[kBlock / 64];
    const uint32_t wave = threadIdx.x >> 6;
    uint32_t carry = 0;
    const uint32_t tiles = launch_tiles(launch_count(P.n_count, P.n));
    for (uint32_t base = 0; base < tiles; base += kBlock) {
        const uint32_t t = base + threadIdx.x;
        const uint32_t v = t < tiles ? P.tile_count[t] : 0u;
        const uint32_t incl = wave_incl_scan(v);
        if (lane_id() == 63) wave_tot[wave] = incl;
        __syncthreads();
        uint32_t before = 0, total = 0;
        #pragma unroll
        for (uint32_t w = 0; w < kBlock / 64; ++w) {
            before += w < wave ? wave_tot[w] : 0u;
            total += wave_tot[w];
        }
        if (t < tiles) P.tile_count[t] = carry + before + (incl - v);
        carry += total;
        __syncthreads();   // wave_tot is rewritten by the next round
    }
    if (threadIdx.x == 0) *P.count = carry;
}

// Words [0, cnt * W) of the tile's destination range, thread after thread.
template <uint32_t W>
__device__ __forceinline__ void compact_copy_words(const float4* src, float4* dst, const uint32_t* sel_idx, size_t first,
                                                   size_t base, uint32_t cnt) {
    for (uint32_t q = threadIdx.x; q < cnt * W; q += kBlock) {
        const uint32_t j = q / W, w = q - j * W;
        dst[(base + j) * W + w] = src[(first + sel_idx[j]) * W + w];
    }
}

__global__ void __launch_bounds__(kBlock) rq_compact_copy(CompactParams P) {
    __shared__ unsigned long long seg_word[kCompactSegs];
    __shared__ uint32_t seg_cnt[kCompactSegs];
    __shared__ uint32_t seg_base[kCompactSegs + 1];
    __shared__ uint32_t sel_idx[kCompactTile];   // the tile's selected records (index within the tile) by rank
    const uint32_t wave = threadIdx.x >> 6;
    const uint32_t tiles = launch_tiles(launch_count(P.n_count, P.n));   // read after the scan wrote *count: the two differ
    for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const size_t first = (size_t)tile * kCompactTile;
        if (threadIdx.x < kCompactSegs) {
            const unsigned long long b = P.bits[(size_t)tile * kCompactSegs + threadIdx.x];
            seg_word[threadIdx.x] = b;
            seg_cnt[threadIdx.x] = (uint32_t)__popcll(b);
        }
        __syncthreads();
        if (threadIdx.x <= kCompactSegs) {
            uint32_t s = 0;
            for (uint32_t q = 0; q < threadIdx.x; ++q) s += seg_cnt[q];
            seg_base[threadIdx.x] = s;
        }
        __syncthreads();
        #pragma unroll
        for (uint32_t k = 0; k < kCompactTile / kBlock; ++k) {
            const uint32_t seg = k * (kBlock / 64) + wave;
            const unsigned long long b = seg_word[seg];   // the ballot rq_compact_count took of this wave's records
            if ((b >> lane_id()) & 1ull) sel_idx[seg_base[seg] + mbcnt64(b)] = k * kBlock + threadIdx.x;   // < cnt <= kCompactTile
        }
        __syncthreads();
        const uint32_t cnt = seg_base[kCompactSegs];
        const size_t base = P.tile_count[tile];   // the tile's offset (rq_compact_scan)
        #pragma unroll
        for (uint32_t s = 0; s < kCompactMaxStreams; ++s) {
            if (s >= P.streams) break;
            switch (P.words[s]) {
                case 1: compact_copy_words<1>(P.src[s], P.dst[s], sel_idx, first, base, cnt); break;
                case 2: compact_copy_words<2>(P.src[s], P.dst[s], sel_idx, first, base, cnt); break;
                case 3: compact_copy_words<3>(P.src[s], P.dst[s], sel_idx, first, base, cnt); break;
                default: compact_copy_words<4>(P.src[s], P.dst[s], sel_idx, first, base, cnt); break;
            }
        }
        if (P.index)
            for (uint32_t j = threadIdx.x; j < cnt; j += kBlock) P.index[base + j] = (uint32_t)(first + sel_idx[j]);
        __syncthreads();   // the LDS arrays are rewritten by the next tile
    }
}

// Blocks of kBlock threads of `Kernel` the chip holds at once (CUs x blocks per CU; 256 x 4 where
// the runtime does not say), found once per process and kernel.
// The cache takes the device that is current at first use.
template <auto Kernel>
unsigned resident_blocks() {
    static const unsigned resident = [] {
        int dev = 0, cus = 256, per = 0;
        if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, Kernel, kBlock, 0) != hipSuccess || per < 1) per = 4;
        return (unsigned)(cus * per);
    }();
    return resident;
}
}  // namespace

unsigned path_resident_blocks() { return resident_blocks<&rq_compact_copy>(); }   // the kernel that holds the most LDS: one figure serves all

void launch_camera(const CamParams& P, unsigned blocks, hipStream_t stream) {
    hipLaunchKernelGGL(rq_camera, dim3(blocks), dim3(kBlock), 0, stream, P);
}
void launch_connect(const ConnectParams& P, unsigned blocks, hipStream_t stream) {
    hipLaunchKernelGGL(rq_connect, dim3(blocks), dim3(kBlock), 0, stream, P);
}
void launch_retire(const RetireParams& P, unsigned blocks, hipStream_t stream) {
    hipLaunchKernelGGL(rq_retire, dim3(blocks), dim3(kBlock), 0, stream, P);
}
void launch_average(const AverageParams& P, unsigned blocks, hipStream_t stream) {
    hipLaunchKernelGGL(rq_average, dim3(blocks), dim3(kBlock), 0, stream, P);
}
void launch_compact(const CompactParams& P, unsigned tile_blocks, hipStream_t stream) {
    hipLaunchKernelGGL(rq_compact_count, dim3(tile_blocks), dim3(kBlock), 0, stream, P);
    hipLaunchKernelGGL(rq_compact_scan, dim3(1), dim3(kBlock), 0, stream, P);
    hipLaunchKernelGGL(rq_compact_copy, dim3(tile_blocks), dim3(kBlock), 0, stream, P);
}

unsigned shade_resident_blocks() { return resident_blocks<&rq_shade<false>>(); }

void launch_shade(const ShParams& P, unsigned blocks, hipStream_t stream) {
    auto kernel = P.randoms ? rq_shade<true> : rq_shade<false>;
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kBlock), 0, stream, P);
}

unsigned resolve_resident_blocks() { return resident_blocks<&rq_resolve<true, true>>(); }   // the variant that holds the most registers: one figure serves all four

void launch_resolve(const DevScene& S, const RsParams& P, unsigned blocks, hipStream_t stream) {
    const bool mat = P.materials != nullptr, tex = S.textured != 0;
    auto kernel = mat ? (tex ? rq_resolve<true, true> : rq_resolve<true, false>)
                      : (tex ? rq_resolve<false, true> : rq_resolve<false, false>);
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kBlock), 0, stream, S, P);
}

unsigned query_resident_blocks() { return resident_blocks<&rq_trace<false, false>>(); }

void launch_query(const DevScene& S, const RqParams& Q, bool any, bool count, unsigned blocks, hipStream_t stream) {
    auto kernel = any ? (count ? rq_trace<true, true> : rq_trace<true, false>)
                      : (count ? rq_trace<false, true> : rq_trace<false, false>);
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kBlock), 0, stream, S, Q);
}

}  // namespace rt
