// rt_wf_schedule.h — how a wavefront frame is scheduled: frames in flight, finish threshold, the
// grid shares of the traversal and finish launches and the finish drain's team size, decided in
// one place from the frame's size.  Plain host C++ (no HIP header), so a test can compile it alone.
#pragma once
#include <stdint.h>

#include <algorithm>

namespace rt {

// The wavefront kernels' scheduling parameters, resolved (rt_tuning in rt_api.h: 0 = default there;
// rt_set_tuning in rt_api.cpp fills these in).  Per context: the library reads no environment variable for them.
struct WfTuning {
    uint32_t tail = 4194304;      // finish threshold one frame at a time (frames in flight: kTailInFlight)
    int refill_min = 8;           // a wave refills once this many of its lanes are idle
    int chunk = 64;               // rays per chunk grab of the traversal kernel
    int fchunk = 64;              // paths per chunk grab of the finish kernel
    int shade_min = 24;           // the finish kernel shades once this many lanes wait
    int shade_min_x = -50;        // the same once its queue ran out (< 0: that percentage of the wave's busy lanes)
    int team = -1;                // finish drain lanes per query (-1: 4 for frames of kTeamAutoMin .. kTeamAutoPaths
                                  // base paths, off otherwise; 0: off; 2 / 4 / 8)
    int finish_frac = 0;          // percent of the resident grid the finish launch takes (0 = by frames in flight)
    int trace_frac = 0;           // percent of the resident grid the bulk wf_trace launches take (0 = by frames in flight)
    int log = 0;                  // 1: per-round queue sizes, stage times and finish diagnostics on stderr;
                                  // 2: also the finish paths' segment counts (one atomic per path)
    bool host_ctl = false;        // host-driven rounds (queue sizes read back every round)
    unsigned shade_blocks = 2048; // wf_shade grid (grid-stride loop), a multiple of 8: 1.6 waves of the resident
                                  // grid leaves CUs to the other frames in flight
};

// default finish threshold with 2 / 3 / 4 frames in flight (C3g sweeps: 1.25M, 1M and 512K paths;
// round 2, with the DP-collapsed tree and the lighter shading kernels, two slots: 2M 5.88 / 5.89,
// 1.57M 5.90 (C3g enters the finish one round earlier between 1.5M and 1.57M live paths),
// 1.5M 5.97 / 6.02, 1M 6.02 / 6.00 Grays/s; four slots serve the small frames of multi-GPU ranks:
// 8-way split 2.92 -> 3.46 Grays/s per rank at 512K against 1M in round 1, 256K-786K within noise
// in round 2, with the finish kernel on 20 % of the grid)
// Final round-2 kernels, 8-way share with four slots: 256K 4.14 / 4.13, 512K 4.25 / 4.26, 768K
// 4.32 / 4.30 Grays/s per rank -> 768K for four slots.
constexpr int kTailInFlightTab[9] = {0, 0, 1310720, 1048576, 786432, 524288, 524288, 524288, 524288};
constexpr int kTailInFlight(int nfl) { return kTailInFlightTab[nfl < 8 ? nfl : 8]; }
// Default frames in flight (render_frame): their buffers, ~300 B per allocated path (pixels x (spp +
// motion-adaptive extra samples)) and slot (128 B path state and ray slots + 176 B of queues), stay
// within kSlotBudget of the 288 GB (1080p x 4 + 2 extra: 3.7 GB a slot; configs[3]'s 3840x2160x16
// frame on one GPU: 40 GB a slot, two slots).
constexpr uint64_t kSlotBudget = 96ull << 30, kSlotBytesPerPath = 300;
// Frames below this many allocated paths keep at most four slots: a configs[0]-sized frame (65K
// paths, ~0.05 ms) on eight slots / eight queues ran bimodally, 2.04-2.10 or 0.55-0.62 Grays/s
// (3 of 6 runs slow), against 2.10-2.54 on four (round 5); the 8-way C3g share (1M paths) gains
// 9 % from eight slots and was steady.  Round 6 traced six such runs (profiles/r06_c1_bimodal.txt):
// the kernels take the same time in slow and fast runs, the slow ones overlap their frames less
// (0.94-1.10 kernels at once against 1.38) -- slot streams sharing hardware queues serialise a
// frame whose GPU work is ~0.12 ms; at four slots there is queue room to spare.
constexpr uint64_t kSmallFramePaths = 1ull << 19;
constexpr uint64_t kSmallShareBasePaths = 2500000;   // see wf_schedule's tail
constexpr int kTailShare = 786432;
// frames of kTeamAutoMin .. kTeamAutoPaths base paths use the finish kernel's team drain by default
// (rt_tuning.team = 0): the C3g rank shares gain, the tiny C1 frame (65K paths) loses 7.5 %
constexpr uint32_t kTeamAutoPaths = 2500000u;
constexpr uint32_t kTeamAutoMin = 262144u;

// A frame's schedule: what run_wavefront copies into the kernels' parameters.
struct WfSchedule {
    int in_flight;             // frames that can overlap this one
    uint32_t tail;             // live paths below which the finish kernel runs the rest
    int trace_frac, finish_frac;   // percent of the resident grid of the bulk wf_trace / the finish launches
    int team;                  // finish drain lanes per query (0: no team drain)
};

// Frames in flight of a frame with `frame_paths` allocated paths (pixels x (spp + extra samples)):
// `requested` when set, else one per slot the hardware queues allow (hw_slots), as many as fit in
// kSlotBudget, at least two.
inline int wf_in_flight(uint64_t frame_paths, int hw_slots, int requested) {
    if (requested > 0) return requested;
    const uint64_t slots = frame_paths < kSmallFramePaths ? std::min(4, hw_slots) : hw_slots;
    return (int)std::max<uint64_t>(2, std::min<uint64_t>(slots, kSlotBudget / (frame_paths * kSlotBytesPerPath + 1)));
}

inline WfSchedule wf_schedule(uint32_t base_paths, int in_flight, int tail_requested, const WfTuning& tu) {
    WfSchedule s;
    s.in_flight = in_flight;
    // finish threshold: with frames in flight the next frames' bulk rounds overlap this
    // frame's tail, so more bulk rounds and a shorter tail pay (kTailInFlight: C3g, 2 in
    // flight 1.25M paths against the one-frame-at-a-time optimum of 4M; 3 in flight 1M)
    int tail = tail_requested ? tail_requested : (in_flight > 1 ? kTailInFlight(in_flight) : 0);
    // eight frames in flight and a frame of at most 2.5M base paths (a multi-GPU rank's share):
    // 768K (round 5, finish on 12 % of the grid: 8-way share 7.02 -> 7.20, 4-way 8.44 -> 8.54
    // Grays/s; 1M hands the 8-way share's whole frame to the finish: 6.08)
    if (!tail_requested && in_flight >= 8 && base_paths <= kSmallShareBasePaths) tail = kTailShare;
    s.tail = tail > 0 ? (uint32_t)tail : tu.tail;
    // the team drain pays where the drain is a large part of the finish: small frames (C3g rank
    // shares, DESIGN.md §3.3: 8-way +2.3 %, 4-way +1.5 %, 2-way ±1 %, the whole 1080p frame four in
    // flight ±0), but not the smallest (C1 256x256x1: -7.5 %)
    s.team = tu.team >= 0 ? tu.team : (base_paths >= kTeamAutoMin && base_paths <= kTeamAutoPaths ? 4 : 0);
    // frames in flight: the finish tail takes part of the resident grid and leaves the rest to the
    // other frames' bulk rounds (C3g sweeps, DESIGN.md §3: two slots 40 %; four or more 20 %: C3g
    // with four slots 20 / 25 / 33 % 8.49-8.54 / 8.21-8.50 / 8.28-8.36 Grays/s, and a multi-GPU
    // rank's share; three 33 %); one frame at a time: all of it
    // four or more frames in flight: the bulk traversal launches take 60 % of the resident grid,
    // leaving CUs to the other frames' kernels (C3g 8.51-8.64 -> 8.61-8.72 Grays/s over five
    // alternating pairs, 75 % +0.5 %; the 8-way rank share at 75 % +0.9 %); fewer frames: all of it
    // eight frames in flight (round 6): the smaller the frame, the smaller the share, so that more
    // frames' bulk rounds run side by side -- 20 % up to 2.5M base paths (8-way C3g rank share 7.26 ->
    // 7.51-7.54 Grays/s, 4-way 8.59 -> 8.87-8.88; 15 % 7.46-7.49), 30 % up to 6M (2-way 9.29 ->
    // 9.47-9.55), 40 % above (the whole C3g frame 9.74-9.83 -> 9.82-9.91; 50 % 9.80-9.81)
    // (profiles/r06_experiments.txt)
    s.trace_frac = tu.trace_frac > 0 ? tu.trace_frac
                 : in_flight >= 8 ? (base_paths <= 2500000u ? 20 : base_paths <= 6000000u ? 30 : 40)
                 : in_flight >= 4 ? 60 : 100;
    // eight frames in flight of at most 6M base paths (a multi-GPU rank's share): 12 % (round 5,
    // after the slots stopped serialising: 8-way rank share 6.76 -> 7.02, 4-way 8.14 -> 8.44, 2-way
    // (4.1M paths) 9.12 -> 9.35 Grays/s; 8 % +-0, 33 % -10 %; the whole C3g frame (8.3M) +-0 and
    // configs[3]'s 16.6M-path rank share -2 %, so larger frames keep 20 %)
    s.finish_frac = tu.finish_frac > 0 ? tu.finish_frac
                  : (in_flight >= 8 && base_paths <= 6000000u) ? 12
                  : in_flight >= 4 ? 20 : in_flight == 2 ? 40 : (in_flight > 1 ? 100 / in_flight : 100);
    return s;
}

}  // namespace rt
