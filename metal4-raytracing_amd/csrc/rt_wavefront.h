// rt_wavefront.h — what the wavefront kernels (rt_wavefront.hip) and the frame scheduler that
// launches them (rt_wavefront_host.cpp) share: the kernels' parameter block, the counter slots the
// host reads or clears, and the table of kernel instances.  Internal to the two files.
#pragma once
#include "rt_kernels.h"

namespace rt {

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

struct WfParams {
    WavefrontBuffers W;
    uint32_t base_paths;   // own pixels * spp
    uint32_t own_pixels;
    uint32_t seg_cap;      // entries per queue segment
    int spp;
    int refill_min;        // wf_trace / wf_finish_step refill once at least this many lanes of a wave are idle
    int chunk;             // wf_trace: rays per chunk grab
    uint32_t tail;         // live paths below which wf_finish_step runs the rest
    uint32_t sort_bins;    // hit-sort bins (0 = shade reads the extend queue unsorted)
    int diag;              // wf_finish_step: record the diagnostics slots (RT_WF_LOG)
    int shade_min;         // wf_finish_step: shade once this many lanes wait (or none traverses)
    int shade_min_x;       // wf_finish_step: the same once the launch's queue is exhausted (< 0: percent of busy lanes)
    int team;              // wf_finish_step: lanes per query in the drain (0: no team drain)
    int fchunk;            // wf_finish_step: paths per chunk grab
    int finish_frac;       // percent of the resident grid the finish launch takes
    int trace_frac;        // percent of the resident grid the bulk wf_trace launches take
    unsigned shade_blocks; // wf_shade grid
    int spans;             // record device-clock launch spans (rt_set_device_spans)
    int dev_ctl;           // device-side control (enqueue_frame): kernels read their queue sizes from
                           // the counters and skip once the live count fell below `tail`
    int finish_q;          // dev_ctl: the finish queue when every enqueued bulk round ran (written by generate)
    const FrameParams* Pd; // this frame's FrameParams in device memory (W.d_params)
    // own pixel index -> image pixel (own_pixel): tiles tile_id % nranks == rank of tile x tile pixels
    FastDiv spp_div, tile_px_div, tiles_x_div;   // by spp, tile * tile, tiles per row
    int tile, rank, nranks;
};

// counter slots (cslot): [q*8 + shard] ray queues q = 0, 1; [16 + shard] shadow queue; [24] extra allocator
constexpr int kCntShadowQ = 16;
constexpr int kCntExtra = 24;
// [66..73] per-XCD chunk counters of the finish launch: XCD k takes chunks k, k + 8, k + 16, ...
// of the finish queue (its long-first order kept chip-wide).  One counter for the whole chip
// serialised the grabs: 3.4M paths in chunks of 32 were ~105K returning atomics on one line.
constexpr int kCntChunkFinish = 66;
constexpr int kCntDiagSegs = 27, kCntDiagIters = 28, kCntDiagTime = 29;   // wf_finish diagnostics
// dev_ctl: [30] tail mode (set by the first extend launch that found fewer than `tail` live
// paths; later bulk launches of the pass return at once), [31] the queue the finish launch reads
constexpr int kCntTailMode = 30, kCntFinishQ = 31;
constexpr int kCntChunkExtend = 32;   // 8 per-XCD chunk counters each
constexpr int kCntChunkConnect = 40;
constexpr int kCntBack = 50;          // the ray queues' back parts (QueueShards in rt_wavefront.hip)

// The kernels of one frame configuration.  count: the traversal statistics counters; full: the
// shading paths needs_full() asks for; sorted: wf_shade reads the hit-sorted queue; team: the
// finish kernel with the team drain.
struct WfKernels {
    using Traverse = void (*)(DevScene, const FrameParams*, WfParams, int cur, int ts);   // ts: device-clock span slot
    using PerEntry = void (*)(DevScene, const FrameParams*, WfParams, int);
    using PerPixel = void (*)(DevScene, const FrameParams*, WfParams);
    using Sort = void (*)(DevScene, WfParams, int cur);
    Traverse extend, connect, finish;   // wf_trace closest hit / any hit, wf_finish_step
    PerEntry shade, extra, resolve;     // (cur), (queue), (with_extra)
    PerPixel generate, motion;
    Sort sort_hist, sort_scatter;
    void (*sort_rowscan)(WfParams);
    // resident blocks (CUs x blocks per CU) of the persistent kernels: the traversal launches
    // (all sized by the plain extend instance) and this finish instance
    unsigned trace_resident, finish_resident;
};
// The first call makes every instance's occupancy query, so call it before a stream is capturing
// (a capture must hold stream work only).
const WfKernels& wf_kernels(bool count, bool full, bool sorted, bool team);

}  // namespace rt
