// rt_wf_counters.h — the one map of WavefrontBuffers::counts and ::tstamp: every word the wavefront
// kernels (rt_wavefront.hip), the frame scheduler (rt_wavefront_host.cpp) and the buffer allocation
// (rt_api_frame.cpp) index.  Plain constants, usable from host-only code; the static_asserts below
// are its test (they hold by compiling).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace rt {

constexpr int kShards = 8;        // queue segments, one per XCD (one allocation counter each)

// ---- counter slots: slot c is word cslot(c), each on a 128-B line of its own, so the per-XCD
// shards never contend for one line's atomics --------------------------------------------------------
constexpr int kCntStride = 32;
constexpr uint32_t cslot(int c) { return (uint32_t)c * kCntStride; }

//                                         slot  length       what
// front parts of ray queues q = 0, 1 ([q * kShards + shard]: QueueShards::L, rt_wf_queue.h)
constexpr int kCntQueue = 0;            //   0   2 * kShards
constexpr int kCntShadowQ = 16;         //  16   kShards      shadow queue
constexpr int kCntExtra = 24;           //  24   1            extra-sample path allocator
                                        //  25   1            unused
constexpr int kCntSorted = 26;          //  26   1            hits the sort kept (misses dropped) = shade's input size
// wf_finish_step diagnostics (RT_WF_LOG): segments of the longest path, iterations and ticks of the slowest wave
constexpr int kCntDiagSegs = 27, kCntDiagIters = 28, kCntDiagTime = 29;   // 27  3
// dev_ctl: tail mode (set by the first extend launch that found fewer than `tail` live paths; later
// bulk launches of the pass return at once), the queue the finish launch reads
constexpr int kCntTailMode = 30, kCntFinishQ = 31;                         // 30  2
constexpr int kCntChunkExtend = 32;     //  32   kShards      per-XCD chunk counters of the extend launches
constexpr int kCntChunkConnect = 40;    //  40   kShards      ... of the connect launches (cleared with the extend ones)
                                        //  48   2            unused
// back parts of the ray queues ([kCntBack + q * kShards + shard]: QueueShards::S)
constexpr int kCntBack = 50;            //  50   2 * kShards
// per-XCD chunk counters of the finish launch: XCD k takes chunks k, k + 8, k + 16, ... of the
// finish queue (its long-first order kept chip-wide).  One counter for the whole chip serialised
// the grabs: 3.4M paths in chunks of 32 were ~105K returning atomics on one line.
constexpr int kCntChunkFinish = 66;     //  66   kShards
constexpr int kCntSlotsWf = 74;         //  74                slots before the diagnostics words

namespace counters_detail {
struct Range {
    int start, len;
};
constexpr Range kSlotRanges[] = {
    {kCntQueue, 2 * kShards}, {kCntShadowQ, kShards},      {kCntExtra, 1},           {kCntSorted, 1},
    {kCntDiagSegs, 1},        {kCntDiagIters, 1},          {kCntDiagTime, 1},        {kCntTailMode, 1},
    {kCntFinishQ, 1},         {kCntChunkExtend, kShards},  {kCntChunkConnect, kShards},
    {kCntBack, 2 * kShards},  {kCntChunkFinish, kShards},
};
// the table is in slot order, no range overlaps the one before it, the last ends inside the slots
constexpr bool disjoint_below(int limit) {
    int end = 0;
    for (const Range& r : kSlotRanges) {
        if (r.start < end || r.len < 1) return false;
        end = r.start + r.len;
    }
    return end <= limit;
}
static_assert(disjoint_below(kCntSlotsWf), "W.counts: counter slot ranges overlap or pass kCntSlotsWf");
// the scheduler clears the extend and connect chunk counters with one memset
static_assert(kCntChunkConnect == kCntChunkExtend + kShards, "chunk counters of extend and connect are one range");
}  // namespace counters_detail

// ---- diagnostics and statistics words, packed after the slots -------------------------------------------
constexpr int kDiagTimeBins = 64;                        // wave end-time / queue-exhaustion histograms: 50 us bins
constexpr uint32_t kDiagTimeBinTicks = 5000;             // 50 us of s_memrealtime ticks (10 ns)
constexpr int kDiagStepBins = 32;                        // steps-per-ray histogram: log2 bins
constexpr int kDiagStepsWords = 2 * kDiagStepBins + 2;   // extend bins, connect bins, the two maxima
constexpr int kDiagLenBounces = 9;                       // entry classes: bounce 0..8 at entry ...
constexpr int kDiagLenClasses = 2 * kDiagLenBounces;     // ... x refracting (tpass > 0) or not
constexpr int kDiagLenBins = 32;                         // segments run in the finish
// kWfStat words.  dev_ctl statistics: rounds run, wf_trace launches run, rays they traced, the extend
// share of those, finish launches
constexpr int kStatRounds = 0, kStatTraceLaunches = 1, kStatTraceRays = 2, kStatExtendRays = 3, kStatFinish = 4;
// wf_finish_step diagnostics (RT_WF_LOG): summed over waves, s_memrealtime ticks (10 ns) spent in
// shading passes and in total, shading passes and lanes shaded
constexpr int kStatDiagShadeT = 5, kStatDiagTotalT = 6, kStatDiagPasses = 7, kStatDiagShaded = 8;
// ... and split at the wave's queue exhaustion: iterations and ticks before / after it, and the
// wave's active lanes summed over its iterations after it
constexpr int kStatDiagItPre = 9, kStatDiagItPost = 10, kStatDiagTPre = 11, kStatDiagTPost = 12, kStatDiagLanesPost = 13;
constexpr int kWfStatWords = 14;
constexpr int kStatDiagWords = kWfStatWords - kStatDiagShadeT;   // the diagnostics part, cleared per finish launch

constexpr int kWfDiagHist = kCntSlotsWf * kCntStride;   // kDiagTimeBins: wf_finish_step wave end times
constexpr int kWfDiagSteps = kWfDiagHist + kDiagTimeBins;   // kDiagStepsWords: wf_trace steps per ray
constexpr int kWfStat = kWfDiagSteps + kDiagStepsWords;     // kWfStatWords: kStat*
// wf_finish_step (RT_WF_LOG=2): paths by segments run in the finish, per entry class
constexpr int kWfDiagLen = kWfStat + kWfStatWords;          // kDiagLenClasses * kDiagLenBins
constexpr int kWfDiagExh = kWfDiagLen + kDiagLenClasses * kDiagLenBins;   // kDiagTimeBins: the waves' queue-exhaustion times
constexpr int kWfCountWords = kCntSlotsWf * kCntStride + kDiagTimeBins + kDiagStepsWords + kWfStatWords +
                              kDiagLenClasses * kDiagLenBins + kDiagTimeBins;
static_assert(kWfCountWords == kWfDiagExh + kDiagTimeBins, "kWfCountWords is the sum of its named parts");
static_assert(kStatDiagLanesPost == kWfStatWords - 1, "kStat* fill kWfStatWords");

// ---- W.tstamp: device-clock launch spans -----------------------------------------------------------
// Launch slots: per pass (base, extra samples) two per round (extend 2k, connect 2k + 1; at most
// kTsRounds rounds) and the finish launch (kTsFinish); the extra pass at kTsPass.
constexpr int kTsRounds = 16;
constexpr int kTsPass = 40, kTsFinish = 33, kTsSlots = 2 * kTsPass;
static_assert(2 * kTsRounds <= kTsFinish && kTsFinish < kTsPass, "launch span slots of a pass overlap");
// a launch slot: its start, then one end word per XCD, each on a 128-B line of its own (the last
// wave of every block takes the max on its XCD's line; one line for all would serialise them)
constexpr int kTsXcds = 8;
constexpr int kTsLine = 16, kTsStride = (1 + kTsXcds) * kTsLine;
// the counter words and, 8-byte aligned after them, the launch spans share one allocation
constexpr size_t kWfTsOffset = ((size_t)kWfCountWords * 4 + 7) / 8 * 8;
constexpr size_t kWfCountAllocBytes = kWfTsOffset + (size_t)kTsSlots * kTsStride * 8;

}  // namespace rt
