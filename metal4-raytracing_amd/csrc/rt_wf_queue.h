// rt_wf_queue.h — the queue layer of the wavefront kernels: how entries are appended to and taken
// from the sharded queues, and the index maths between path ids, pixels and queue entries.
//
// Queues are split into kShards segments; a block appends to segment blockIdx % 8 with ONE
// returning atomic per 256 entries (wave ballot + LDS prefix), so no counter word sees more
// than ~1/2048 of the entries (one word serialises at ~88 atomics/us, MI355X_MICROARCH.md
// 'dequeue').  Grids are multiples of 8, so segment k only receives chunks c == k (mod 8) and
// a segment of n/8 + 4096 (+ 256 per extra sample) entries can never overflow
// (wavefront_queue_entries, rt_wavefront_host.cpp, sizes them).
//
// A ray queue's shard k holds L[k] entries at the front of its segment (ascending) and S[k] at the
// back (descending from seg_cap - 1): wf_shade appends the continuation rays of paths that have
// refracted (likely_long) at the front and the rest at the back, so the finish kernel, which
// takes the queue front parts first, starts the long glass paths before the short ones (they
// would otherwise set the end of its launch).  Primary rays (generate, extra samples) go to the
// front.  Counters: L in [q * 8 + k], S in [kCntBack + q * 8 + k] (rt_wf_counters.h).
//
// The pure index functions (RT_HD) also compile for the host: tools/wf_queue_check.cpp,
// tests/test_wf_queue.py.  The rest is device code.
#pragma once
#include "rt_math.h"
#include "rt_wf_counters.h"

namespace rt {

// ---- index maths (host and device) ---------------------------------------------------------------
// n / d for 32-bit n by a multiply-high and two shifts (Granlund, Montgomery, PLDI 1994, fig. 4.1):
// the path-id -> pixel mappings run per refill / per shaded hit, where an integer division by a
// run-time divisor costs ~30 VALU instructions
struct FastDiv {
    uint32_t d, m, s1, s2;
};
inline FastDiv make_fastdiv(uint32_t d) {
    FastDiv f;
    f.d = d;
    uint32_t l = 0;
    while (l < 32 && (1ull << l) < d) ++l;
    f.m = (uint32_t)(((1ull << 32) * ((1ull << l) - d)) / d + 1);
    f.s1 = l < 1 ? l : 1;
    f.s2 = l > 1 ? l - 1 : 0;
    return f;
}
RT_HD uint32_t fdiv(uint32_t n, const FastDiv& f) {   // n / f.d (make_fastdiv)
    const uint32_t t = umulhi32(f.m, n);
    return (t + ((n - t) >> f.s1)) >> f.s2;
}

RT_HD uint32_t compact1by1(uint32_t x) {
    x &= 0x55555555u;
    x = (x | (x >> 1)) & 0x33333333u;
    x = (x | (x >> 2)) & 0x0f0f0f0fu;
    x = (x | (x >> 4)) & 0x00ff00ffu;
    x = (x | (x >> 8)) & 0x0000ffffu;
    return x;
}

// own pixel index -> image pixel: tiles tile_id % nranks == rank of tile x tile pixels (the tail of WfParams)
struct PixelMap {
    FastDiv spp_div, tile_px_div, tiles_x_div;   // by spp (path id -> own pixel), tile * tile, tiles per row
    int tile, rank, nranks;
};
// own pixel index -> image coordinates (tiles tile_id % nranks == rank, Morton order in a tile)
RT_HD void own_pixel(const PixelMap& M, uint32_t i, int& px, int& py) {
    const uint32_t T = (uint32_t)M.tile;
    const uint32_t k = fdiv(i, M.tile_px_div), r = i - k * M.tile_px_div.d;
    const uint32_t tid = (uint32_t)M.rank + k * (uint32_t)M.nranks;
    const uint32_t ty = fdiv(tid, M.tiles_x_div), tx = tid - ty * M.tiles_x_div.d;
    uint32_t lx, ly;
    if ((T & (T - 1)) == 0) {
        lx = compact1by1(r);
        ly = compact1by1(r >> 1);
    } else {
        lx = r % T;
        ly = r / T;
    }
    px = (int)(tx * T + lx);
    py = (int)(ty * T + ly);
}

// A path's state bits in its queue entry (d.w): bounce | tpass << 8 | step << 16
struct PathState {
    int bounce, tpass, step;
};
RT_HD uint32_t pack_state(int bounce, int tpass, int step) {
    return (uint32_t)bounce | ((uint32_t)tpass << 8) | ((uint32_t)step << 16);
}
RT_HD PathState unpack_state(uint32_t s) {
    PathState r;
    r.bounce = (int)(s & 0xffu);
    r.tpass = (int)((s >> 8) & 0xffu);
    r.step = (int)(s >> 16);
    return r;
}

// The front (L) and back (S) entry counts of a ray queue's shards, clamped to the segment.
struct QueueShards {
    uint32_t L[kShards], S[kShards];
};
RT_HD uint32_t queue_len(const QueueShards& qs) {
    uint32_t n = 0;
    #pragma unroll
    for (int k = 0; k < kShards; ++k) n += qs.L[k] + qs.S[k];
    return n;
}
// shard-local index g (< L + S) -> position in the shard's segment
RT_HD uint32_t seg_pos(uint32_t g, uint32_t l, uint32_t seg_cap) {
    return g < l ? g : seg_cap - 1u - (g - l);
}
// dense consumer index g (< queue_len) -> entry index: the front parts of all shards first, then the back parts
RT_HD uint32_t dense_entry(const QueueShards& qs, uint32_t g, uint32_t seg_cap) {
    uint32_t ltot = 0;
    #pragma unroll
    for (int k = 0; k < kShards; ++k) ltot += qs.L[k];
    const bool back = g >= ltot;
    if (back) g -= ltot;
    uint32_t k = 0, start = 0, acc = 0;
    #pragma unroll
    for (int j = 0; j < kShards - 1; ++j) {
        acc += back ? qs.S[j] : qs.L[j];
        const bool past = g >= acc;
        k = past ? (uint32_t)(j + 1) : k;
        start = past ? acc : start;
    }
    const uint32_t i = g - start;
    return k * seg_cap + (back ? seg_cap - 1u - i : i);
}

}  // namespace rt

// ---- device code -------------------------------------------------------------------------------------
#if defined(__HIPCC__)
#include "rt_device.h"

namespace rt {

__device__ __forceinline__ uint32_t lane_id() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }
__device__ __forceinline__ uint32_t mbcnt64(unsigned long long m) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v) {
    const uint32_t lane = lane_id();
    #pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t t = __shfl_up(v, off, 64);
        if (lane >= (uint32_t)off) v += t;
    }
    return v;
}

// Block-wide prefix over the waves: each wave's `writer` lane stores the wave's total in w[wave]
// (one word per wave); after one barrier every thread has the sum of the waves before its own and
// the block's total.  w must not be written again before every wave has read it: a caller in a
// loop alternates two arrays (wf_shade's ring fill) or has a barrier of its own in between.
template <int WAVES>
__device__ __forceinline__ void block_prefix(bool writer, uint32_t wave_total, uint32_t* w, uint32_t& base,
                                             uint32_t& total) {
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (writer) w[wave] = wave_total;
    __syncthreads();
    base = 0;
    total = 0;
    #pragma unroll
    for (uint32_t j = 0; j < (uint32_t)WAVES; ++j) {
        const uint32_t c = w[j];
        base += j < wave ? c : 0u;
        total += c;
    }
}

// Block-aggregated allocation from a counter: the waves' totals to LDS, ONE returning atomic by
// thread 0 for the block's total, then every wave reads where its share starts.  It does not use
// block_prefix: handing the atomic's result to the other waves through the same four words takes
// the second barrier anyway, so thread 0 makes the prefix on the way.  Every thread of the block
// calls it (converged loop); three barriers, the last so that sh can be used again at once.
struct BlockAlloc {
    uint32_t w[kBlock / 64];
};
static_assert(kBlock / 64 == 4, "block_alloc_base: four waves per block");
__device__ __forceinline__ uint32_t block_alloc_base(bool writer, uint32_t wave_total, uint32_t* counter, BlockAlloc& sh) {
    const int wave = threadIdx.x >> 6;
    if (writer) sh.w[wave] = wave_total;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t c0 = sh.w[0], c1 = sh.w[1], c2 = sh.w[2], c3 = sh.w[3];
        uint32_t tot = c0 + c1 + c2 + c3;
        uint32_t b = tot ? atomicAdd(counter, tot) : 0u;
        sh.w[0] = b;
        sh.w[1] = b + c0;
        sh.w[2] = b + c0 + c1;
        sh.w[3] = b + c0 + c1 + c2;
    }
    __syncthreads();
    const uint32_t r = sh.w[wave];
    __syncthreads();
    return r;
}
// one slot for every thread with pred (ballot: no scan)
__device__ __forceinline__ uint32_t block_alloc(bool pred, uint32_t* counter, BlockAlloc& sh) {
    const unsigned long long m = __ballot(pred);
    return block_alloc_base(lane_id() == 0, (uint32_t)__popcll(m), counter, sh) + mbcnt64(m);
}
// v slots per thread (wave scan)
__device__ __forceinline__ uint32_t block_alloc_n(uint32_t v, uint32_t* counter, BlockAlloc& sh) {
    const uint32_t incl = wave_incl_scan(v);
    return block_alloc_base(lane_id() == 63, incl, counter, sh) + incl - v;
}

// Three block-aggregated allocations at once (wf_shade: pr[0] shadow ray, pr[1] front / pr[2] back
// continuation ray), one returning global atomic per part and block, with the continuation rays
// grouped by the direction octant `oct` (3 bits) inside each part's range: a per-block counting
// sort of the appends through LDS atomics (the rank inside an octant is arbitrary), no separate
// sort pass.
struct BlockAllocOct {
    uint32_t cnt[3][8];    // shadow uses [0][0]
    uint32_t base[3][8];
};
__device__ __forceinline__ void block_alloc3_oct(const bool (&pr)[3], uint32_t oct, uint32_t* const (&ctr)[3],
                                                 BlockAllocOct& sh, uint32_t (&out)[3]) {
    if (threadIdx.x < 24) (&sh.cnt[0][0])[threadIdx.x] = 0u;
    __syncthreads();
    uint32_t rank[3] = {0u, 0u, 0u};
    #pragma unroll
    for (int i = 0; i < 3; ++i)
        if (pr[i]) rank[i] = atomicAdd(&sh.cnt[i][i ? oct : 0u], 1u);
    __syncthreads();
    if (threadIdx.x < 3) {
        const int i = threadIdx.x;
        uint32_t tot = 0, pre[8];
        #pragma unroll
        for (int o = 0; o < 8; ++o) { pre[o] = tot; tot += sh.cnt[i][o]; }
        const uint32_t b = tot ? atomicAdd(ctr[i], tot) : 0u;
        #pragma unroll
        for (int o = 0; o < 8; ++o) sh.base[i][o] = b + pre[o];
    }
    __syncthreads();
    #pragma unroll
    for (int i = 0; i < 3; ++i) out[i] = sh.base[i][i ? oct : 0u] + rank[i];
    __syncthreads();
}

// Inclusive prefix of a sharded queue's segment counts, loaded once per kernel (uniform, so the
// loads are scalar and the lookups below stay in registers).
struct ShardPrefix {
    uint32_t end[kShards];
};
__device__ __forceinline__ ShardPrefix load_prefix(const uint32_t* cnt, uint32_t cap = 0xffffffffu) {
    ShardPrefix p;
    uint32_t acc = 0;
    #pragma unroll
    for (int k = 0; k < kShards; ++k) {
        acc += min(__builtin_amdgcn_readfirstlane(cnt[cslot(k)]), cap);   // a counter may run past a full segment
        p.end[k] = acc;
    }
    return p;
}
__device__ __forceinline__ QueueShards load_queue(const uint32_t* counts, int q, uint32_t seg_cap) {
    QueueShards r;
    #pragma unroll
    for (int k = 0; k < kShards; ++k) {
        const uint32_t l = min(__builtin_amdgcn_readfirstlane(counts[cslot(q * kShards + k)]), seg_cap);
        r.L[k] = l;
        r.S[k] = min(__builtin_amdgcn_readfirstlane(counts[cslot(kCntBack + q * kShards + k)]), seg_cap - l);
    }
    return r;
}

// a 16-B load of data read once (nontemporal: it does not displace the lines gathered beside it).
// wf_shade and the finish refill read their queue entries this way; wf_trace (extend) does not
// (wf_shade reads the same entries again: nontemporal extend loads slowed it, round 4)
__device__ __forceinline__ float4 ld_stream(const float4* p) {
    typedef float v4f __attribute__((ext_vector_type(4)));
    const v4f v = __builtin_nontemporal_load(reinterpret_cast<const v4f*>(p));
    return make_float4(v.x, v.y, v.z, v.w);
}

}  // namespace rt
#endif
