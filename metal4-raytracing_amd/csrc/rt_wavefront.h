// rt_wavefront.h — the wavefront pipeline's interface.  For the API files: the buffers of a frame
// slot, a frame's statistics and timeline, run_wavefront / wavefront_collect.  For the kernels
// (rt_wavefront.hip) and the frame scheduler that launches them (rt_wavefront_host.cpp): the
// kernels' parameter block and the table of kernel instances.  The counter words: rt_wf_counters.h.
#pragma once
#include <vector>

#include "rt_kernels.h"
#include "rt_wf_counters.h"
#include "rt_wf_queue.h"
#include "rt_wf_schedule.h"

namespace rt {

// Wavefront pipeline (rt_wavefront.hip): path state SoA indexed by path id
// (own pixel index * spp + sample; extra samples after base_paths), ray queues of
// {float4 o (w = path id), float4 d}, hit records {t, tri id, u, v}, shadow queue of
// {float4 o (w = path id), float4 d (w = tmax), float4 contribution (w = root word)}.
struct WavefrontBuffers {
    size_t queue_entries = 0;     // kShards segments of queue_entries / kShards
    float4* p_accum = nullptr;
    uint4* p_meta = nullptr;      // extra-sample paths only: (pixel, sample, 0, halton index)
    // ray queues: entry e = {origin, w = path id}, {direction, w = path state bits: bounce | tpass << 8 |
    // step << 16}; qc[q][e] = the path's throughput colour (absent for state 0, the primary ray: 1)
    float4* q[2] = {nullptr, nullptr};
    float4* qc[2] = {nullptr, nullptr};
    // qr[q][e] = the entry's root word (rt_device.h root_word): every producer writes it with the
    // entry, 0 where it supplies none; a shadow ray's is the w of its third record
    uint32_t* qr[2] = {nullptr, nullptr};
    float4* hits = nullptr;
    float4* sq = nullptr;
    uint32_t* counts = nullptr;   // device counter words (the map: rt_wf_counters.h)
    uint32_t* h_counts = nullptr; // pinned host mirror
    // device-clock launch spans (kTsSlots launch slots x kTsStride words, s_memrealtime) + pinned mirror
    unsigned long long* tstamp = nullptr;
    unsigned long long* h_tstamp = nullptr;
    uint2* px_extra = nullptr;    // per own pixel: (first extra path - base_paths, count)
    // per-bounce hit sort (wf_sort_*): the hits reordered by key as {o, d, hit, colour} float4 quads,
    // per-(bin, block) counts, per-bin totals
    float4* sorted = nullptr;
    uint32_t* sort_table = nullptr;
    uint32_t* sort_total = nullptr;
    size_t cap_paths = 0;         // base + extra paths
    size_t cap_pixels = 0;
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    // FrameParams of the frame in flight: one device copy the kernels read, uploaded from a ring
    // of pinned host slots
    static constexpr int kParamSlots = 4;
    FrameParams* d_params = nullptr;
    FrameParams* h_params = nullptr;
    hipEvent_t param_ev[kParamSlots] = {nullptr, nullptr, nullptr, nullptr};
    int param_slot = 0;
};
// Hit sort: kSortBlocks blocks of kSortThreads share one partition of the queue in the histogram
// and scatter kernels; bins are a power of two in [kSortMinBins, kSortMaxBins].
constexpr int kSortBlocks = 256;
constexpr int kSortThreads = 1024;
constexpr int kSortMinBins = 1024;
constexpr int kSortMaxBins = 4096;
constexpr int kSortBinsDefault = 0;   // off: measured slower on C3g (DESIGN.md §3 'Hit sort')
// Per-frame measurements of the wavefront pipeline. stage_ms: [0] generate, [1] extend,
// [2] shade, [3] connect, [4] resolve (+extra-sample bookkeeping), [5] finish, [6] hit sort.
struct WfFrameStats {
    float trace_dev_ms, finish_dev_ms;   // device-clock spans of the extend + connect / finish launches
    int trace_dev_launches, finish_dev_launches;
    float stage_ms[7];
    int iterations;
    unsigned long long trace_rays;  // rays traced by wf_trace launches (extend + connect)
    unsigned long long trace_closest_rays;   // the extend share
    int trace_launches;
    float trace_ms;                 // their summed device time
    int finish_launches;
    int graph_mode;                 // kGraph*: how the frame was submitted
};
// Host-side record of a frame enqueued with device-side control: events between the launches and
// which stage each interval belongs to; collected once the frame is done (wavefront_collect).
struct WfTimeline {
    static constexpr int kMaxEv = 160;
    struct Span {
        int stage, a, b;
    };
    hipEvent_t ev[kMaxEv] = {};
    Span spans[kMaxEv];
    int n_ev = 0, n_spans = 0;
    bool pending = false;
    bool dev_spans = false;   // the frame recorded device-clock launch spans (tstamp copied back)
    // RT_GRAPH: the slot's frame captured as two HIP graphs (events recorded as external event
    // nodes, so the spans above keep timing it) and replayed while `key` (every launch argument and
    // enqueue decision of the frame) is unchanged: exec[0] up to the motion vectors, exec[1] the
    // rest, with the wait for the previous frame enqueued between them (a plain stream wait, not a
    // captured external-event wait node)
    hipGraphExec_t exec[2] = {nullptr, nullptr};
    std::vector<uint8_t> key;
    bool graph_failed = false;   // capture was refused once: this slot stays eager
    int graph_mode = 0;          // the pending frame: kGraph* (rt_stats total_graph_*)
};
constexpr int kGraphEager = 0, kGraphReplay = 1, kGraphCapture = 2, kGraphFallback = 3;
// One wavefront frame of `own_tiles` tiles on `stream` (rt_wavefront_host.cpp); false on a HIP
// error (*err).  Device-driven rounds, the default, enqueue the whole frame and return: `tl`
// receives the timeline and wavefront_collect fills the stats once the stream has finished;
// graphs: as two replayed HIP graphs.  Host-driven rounds (tu.host_ctl or tu.log set, no `tl`, or
// a finish threshold <= 1) read the queue sizes back every round; *fs is complete on return.
// sched: the finish threshold, grid shares and team drain (wf_schedule, rt_wf_schedule.h).
// count: the traversal statistics counters; spans: device-clock launch spans.  sort_bins: hit-sort
// bins (0 = no sort).  extra_pass: the motion-adaptive extra samples can be non-zero this frame
// (something moved in this or the previous frame); device-driven rounds skip their pass otherwise.
// prev_done (may be null): the previous frame, in flight on another stream; the extra-sample pass
// and the resolve (which read its accumulation and motion outputs) are ordered after it,
// everything before them overlaps it.
bool run_wavefront(const DevScene& S, const FrameParams& P, WavefrontBuffers& W, const WfTuning& tu,
                   const WfSchedule& sched, int own_tiles, bool count, bool spans, int sort_bins, bool extra_pass,
                   hipStream_t stream, hipEvent_t prev_done, WfTimeline* tl, WfFrameStats* fs, const char** err,
                   bool graphs = true);
bool wavefront_collect(const WavefrontBuffers& W, WfTimeline& T, WfFrameStats* fs, const char** err);
size_t wavefront_queue_entries(size_t paths, int max_extra);


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
    int count;             // the frame runs the counting instances: producers count a retired ray's root visit
    int finish_q;          // dev_ctl: the finish queue when every enqueued bulk round ran (written by generate)
    const FrameParams* Pd; // this frame's FrameParams in device memory (W.d_params)
    PixelMap px;           // path id -> own pixel -> image pixel (own_pixel, rt_wf_queue.h)
};

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
