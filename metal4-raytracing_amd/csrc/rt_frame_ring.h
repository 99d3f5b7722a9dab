// rt_frame_ring.h — the bookkeeping of frames in flight: which slot a frame takes and which
// earlier frame it waits for, the geometry generations updates and frames rotate over, the motion
// and accumulation targets a frame reads and writes.  The decisions only: every function here says
// what to wait for or what to use, and rt_api_frame.cpp / rt_api_scene.cpp issue the HIP calls.
// Plain host C++ (no HIP header), so a test can compile it alone (tools/frame_ring_print.cpp).
#pragma once
#include <stdint.h>

#include <algorithm>

namespace rt {

#ifndef RT_MAX_SLOTS
#define RT_MAX_SLOTS 8
#endif
constexpr int kMaxSlots = RT_MAX_SLOTS;
constexpr int kGens = kMaxSlots;   // generations allocated at most (ngens of them in use)
// Motion vectors rotate over kMaxSlots + 1 targets: a wavefront frame writes target m + 1 and
// reads the previous frame's target m, so it never overwrites a target an older frame still in
// flight reads (the megakernel reads and rewrites target m in place).
constexpr int kMotionTargets = kMaxSlots + 1;

// What rt_render_frame does for the next frame, in this order: wait for (harvest) the frame
// `slot` last held; the stream waits retile_wait and ctx_wait; record the update stream's event
// on `flip`; `drain`; with `regen`, free the generations from `ngens` on; begin_frame; fill the
// parameters and launch, with the wait for `prev` where `cross` says; commit_frame.
struct FramePlan {
    int nfl;             // frames in flight, as given
    int tiles[3];        // tile_size, rank, nranks, as given
    int slot;            // the slot (and stream) the frame takes
    int prev;            // the slot of the previous frame
    bool cross;          // the previous frame runs on another stream (or a pack / unpack extended it): this
                         // frame's history inputs (the accumulation target and motion vectors it wrote)
                         // are read after its `done`
    bool retile_wait;    // a pack / unpack of the previous frame on another stream, and another tile set:
                         // the whole frame follows prev's `done` (the tiles this frame owns are disjoint
                         // from the ones the pack read or the unpack wrote unless the tile set changed)
    bool ctx_wait;       // the slot's stream first waits for the work enqueued on the context's stream
    bool flip;           // updates went into the next generation: this frame reads it
    // another number of frames in flight than the previous frame's (a new frame size or tile set):
    // the frames in flight finish first, then the geometry rotates over max(2, nfl) generations
    // from the current one, and the generations past them are freed
    bool regen;          // the number changed
    bool drain;          // ... and there are frames to finish (not before the first frame)
    int ngens;           // generations in rotation from this frame on
    int gen;             // the generation the frame reads
    int motion_prev, motion_out;   // motion targets read and written
};

// Before a geometry update.  seed: the first update since the newest frame; it waits for the frames
// of wait[k] (they still read generation dst), then copies generation src into dst.  Every update
// until the next frame writes dst.
struct UpdatePlan {
    bool seed;
    int src, dst;
    bool wait[kMaxSlots];
};

struct FrameRing {
    struct Slot {
        bool used = false;       // holds a frame (since rt_resize)
        int gen = 0;             // geometry generation the frame reads
        uint64_t ctx_seen = 0;   // ctx_work the slot's stream last waited for
        uint64_t seq = 0;        // frame number (harvest order)
    };
    Slot slot[kMaxSlots];
    uint64_t frame_no = 0;           // frames submitted since rt_resize
    int last_slot = 0;               // slot of the newest frame
    bool tiles_pending = false;      // a pack / unpack extended the newest frame's `done`
    int last_tiles[3] = {0, 0, 0};   // tile_size, rank, nranks of the newest frame
    int cur_nfl = 0;                 // frames in flight of the newest frame (a change drains and re-sizes the rotation)
    // Per-frame geometry in generations used round robin: frames read generation `gcur`; the first
    // update after a frame copies it into the next generation (once the frames still reading that
    // one, ngens frames back, have finished) and every update until the next frame writes there, so
    // frames in flight keep their geometry while the next frame's is built.  ngens = max(2, frames
    // in flight): with an update before every frame (skinning, refit), all frames in flight still
    // overlap, and no more copies exist than frames can read.
    int gcur = 0;          // generation new frames read
    int ngens = 2;         // generations in rotation
    bool gdirty = false;   // updates since the newest frame went into generation next_gen()
    int motion_cur = 0;    // motion target the newest frame wrote
    int read_idx = 0;      // accumulation target that holds the history (the other one is written)
    uint64_t ctx_work = 1; // bumped whenever work that frames must follow is enqueued on the context's stream

    int next_gen() const { return (gcur + 1) % ngens; }
    int write_gen() const { return gdirty ? next_gen() : gcur; }   // the generation updates and builds write

    // wavefront: the frame runs the wavefront pipeline (else the megakernel, with nfl == 1)
    FramePlan plan_frame(int nfl, bool wavefront, int tile_size, int rank, int nranks) const {
        FramePlan p;
        p.nfl = nfl;
        p.tiles[0] = tile_size, p.tiles[1] = rank, p.tiles[2] = nranks;
        p.slot = frame_no > 0 ? (last_slot + 1) % nfl : 0;
        p.prev = last_slot;
        const bool prev_used = slot[last_slot].used;
        p.cross = frame_no > 0 && prev_used && (last_slot != p.slot || tiles_pending);
        const bool retile = tile_size != last_tiles[0] || rank != last_tiles[1] || nranks != last_tiles[2];
        p.retile_wait = tiles_pending && retile && prev_used;
        // Only when the slot has not yet waited for that work: an event recorded on the context's
        // stream also covers the frame slot 0 has in flight there, and waiting on it every frame held
        // each slot-1..3 frame until that frame had finished (the four slots ran in batches; C3g, 20
        // steps: 3.64 ms per step).
        p.ctx_wait = p.slot != 0 && slot[p.slot].ctx_seen != ctx_work;
        p.flip = gdirty;
        p.gen = write_gen();
        p.regen = nfl != cur_nfl;
        p.drain = p.regen && cur_nfl != 0;
        p.ngens = p.regen ? std::max(std::max(2, nfl), p.gen + 1) : ngens;
        p.motion_prev = motion_cur;
        p.motion_out = wavefront ? (motion_cur + 1) % kMotionTargets : motion_cur;
        return p;
    }
    // Once the plan's waits are issued: what holds even if submitting the frame then fails.
    void begin_frame(const FramePlan& p) {
        slot[p.slot].ctx_seen = ctx_work;
        gcur = p.gen;
        gdirty = false;
        ngens = p.ngens;
        cur_nfl = p.nfl;
    }
    // The frame is enqueued.
    void commit_frame(const FramePlan& p) {
        Slot& s = slot[p.slot];
        s.used = true;
        s.seq = frame_no;
        s.gen = gcur;
        last_slot = p.slot;
        frame_no += 1;
        tiles_pending = false;
        for (int i = 0; i < 3; ++i) last_tiles[i] = p.tiles[i];
        motion_cur = p.motion_out;
        read_idx = 1 - read_idx;   // swap accumulationTargets (Renderer.swift:1492-1494)
    }

    UpdatePlan plan_update() const {
        UpdatePlan u;
        u.seed = !gdirty;
        u.src = gcur;
        u.dst = next_gen();
        for (int k = 0; k < kMaxSlots; ++k) u.wait[k] = u.seed && slot[k].used && slot[k].gen == u.dst;
        return u;
    }
    void commit_update() { gdirty = true; }

    // A pack / unpack was enqueued after the newest frame (none: nothing to extend), on the
    // context's stream or on a caller's: it waits for that frame's `done` and records it again
    // after itself, so the frame that next writes the same accumulation target waits for it too.
    bool newest_used() const { return slot[last_slot].used; }
    void tiles_enqueued(bool ctx_stream) {
        if (ctx_stream) ctx_work++;
        if (newest_used()) tiles_pending = true;
    }

    // rt_resize (after a drain): new targets, no frame holds a slot.  The generations, the tile set
    // and the frames in flight of the last frame stay.
    void reset_targets() {
        for (Slot& s : slot) s.used = false;
        frame_no = 0;
        last_slot = 0;
        motion_cur = 0;
        read_idx = 0;
    }

    // rt_wait: the slots oldest frame first, so that the statistics end on the newest one.
    void harvest_order(int order[kMaxSlots]) const {
        for (int k = 0; k < kMaxSlots; ++k) order[k] = k;
        std::sort(order, order + kMaxSlots, [this](int a, int b) { return slot[a].seq < slot[b].seq; });
    }
};

}  // namespace rt
