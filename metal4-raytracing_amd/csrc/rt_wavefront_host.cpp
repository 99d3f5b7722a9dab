// rt_wavefront_host.cpp — the wavefront frame scheduler: how one frame becomes launches of the
// kernels in rt_wavefront.hip.  Host-driven rounds read every round's queue size back
// (RT_WF_HOST=1 / RT_WF_LOG=1, and the bulk-only test configuration tail <= 1); device-driven
// rounds, the default, enqueue the whole frame at once, eagerly or as two replayed HIP graphs.
// What the launches get of the machine (finish threshold, grid shares, team drain) is decided
// before, in rt_wf_schedule.h.
#include "rt_shade.h"
#include "rt_wavefront.h"

#include <atomic>
#include <cstdio>
#include <cstring>
#include <vector>

namespace rt {

// Segment k only receives entries from blocks b == k (mod 8): at most n/8 + 256 per pass over n
// inputs, and (own pixels/8 + 256) * maxExtra from the extra-sample pass (the bound: rt_wf_queue.h).
size_t wavefront_queue_entries(size_t paths, int max_extra) {
    return (size_t)kShards * (paths / kShards + 4096 + 256 * (size_t)max_extra);
}

// false, and *err = "<what>: <HIP's message>" (one buffer per thread), unless e is hipSuccess
static bool hip_ok(hipError_t e, const char* what, const char** err) {
    if (e == hipSuccess) return true;
    static thread_local char msg[192];
    snprintf(msg, sizeof msg, "%.120s: %s", what, hipGetErrorString(e));
    *err = msg;
    return false;
}
#define WF_CHECK(expr) do { if (!hip_ok((expr), #expr, err)) return false; } while (0)

namespace {

unsigned grid_for(uint32_t n, unsigned cap) {
    unsigned g = (unsigned)(((uint64_t)n + kBlock - 1) / kBlock);
    if (g > cap) g = cap;
    g = (g + kShards - 1) / kShards * kShards;  // multiple of 8: segment bound (see rt_wf_queue.h)
    return g == 0 ? kShards : g;
}

uint32_t queue_total(const uint32_t* h, int q) {   // q = 0, 1: a ray queue (both ends); 2: the shadow queue
    uint32_t s = 0;
    for (int k = 0; k < kShards; ++k) s += h[cslot(q * kShards + k)] + (q < 2 ? h[cslot(kCntBack + q * kShards + k)] : 0u);
    return s;
}

int rounds_for(uint64_t paths, uint32_t tail) {
    if (paths < tail) return 0;
    int k = 2;
    while (k < kTsRounds && (paths >> (k - 1)) >= tail) ++k;
    return k;
}

// ---- RT_WF_LOG output of the host-driven rounds (h: the counters read back after the launch) ------
void print_finish_diag(const uint32_t* h, int it, uint32_t n, float ms) {
    fprintf(stderr, "[wf] it %d finish paths %u  %.3f ms; longest path %u segments, "
            "slowest wave %u iterations in %.3f ms\n", it, n, ms, h[cslot(kCntDiagSegs)],
            h[cslot(kCntDiagIters)], h[cslot(kCntDiagTime)] * 1e-5);
    const double st = h[kWfStat + kStatDiagShadeT], tt = h[kWfStat + kStatDiagTotalT];
    const double np = h[kWfStat + kStatDiagPasses], ns = h[kWfStat + kStatDiagShaded];
    fprintf(stderr, "[wf] finish: %.1f %% of wave time in shading passes, %.0f passes, %.1f lanes per pass\n",
            tt > 0 ? 100.0 * st / tt : 0.0, np, np > 0 ? ns / np : 0.0);
    for (int cl = 0; cl < kDiagLenClasses; ++cl) {
        uint32_t tot = 0;
        double sum = 0;
        for (int b = 0; b < kDiagLenBins; ++b) {
            tot += h[kWfDiagLen + cl * kDiagLenBins + b];
            sum += (double)b * h[kWfDiagLen + cl * kDiagLenBins + b];
        }
        if (!tot) continue;
        fprintf(stderr, "[wf] finish paths entering at bounce %d%s: %u, segments mean %.2f:", cl % kDiagLenBounces,
                cl >= kDiagLenBounces ? " refracting" : "", tot, sum / tot);
        for (int b = 0; b < kDiagLenBins; ++b)
            if (h[kWfDiagLen + cl * kDiagLenBins + b]) fprintf(stderr, " %d:%u", b, h[kWfDiagLen + cl * kDiagLenBins + b]);
        fprintf(stderr, "\n");
    }
    fprintf(stderr, "[wf] finish wave end times (50 us bins):");
    for (int b = 0; b < kDiagTimeBins; ++b)
        if (h[kWfDiagHist + b]) fprintf(stderr, " %d:%u", b, h[kWfDiagHist + b]);
    fprintf(stderr, "\n[wf] finish queue exhausted at (50 us bins):");
    for (int b = 0; b < kDiagTimeBins; ++b)
        if (h[kWfDiagExh + b]) fprintf(stderr, " %d:%u", b, h[kWfDiagExh + b]);
    const double ip = h[kWfStat + kStatDiagItPre], ix = h[kWfStat + kStatDiagItPost];
    const double tp = h[kWfStat + kStatDiagTPre], tx = h[kWfStat + kStatDiagTPost];
    const double lx = h[kWfStat + kStatDiagLanesPost];
    double waves = 0;
    for (int b = 0; b < kDiagTimeBins; ++b) waves += h[kWfDiagHist + b];
    waves = waves > 0 ? waves : 1;
    fprintf(stderr, "\n[wf] finish per wave: %.0f iterations at %.2f us before its queue ran out, %.0f at %.2f us "
            "after (%.1f active lanes)\n", ip / waves, ip > 0 ? tp * 0.01 / ip : 0.0, ix / waves,
            ix > 0 ? tx * 0.01 / ix : 0.0, ix > 0 ? lx / ix : 0.0);
}

// ms: extend, sort, shade, connect
void print_round_diag(const uint32_t* h, int it, uint32_t n, const float (&ms)[4], bool count) {
    fprintf(stderr, "[wf] it %d rays %u shadow %u  extend %.3f sort %.3f shade %.3f connect %.3f ms\n", it, n,
            queue_total(h, 2), ms[0], ms[1], ms[2], ms[3]);
    if (!count) return;
    for (int any = 0; any < 2; ++any) {
        fprintf(stderr, "[wf]   %s steps/ray log2 bins (max %u):", any ? "connect" : "extend", h[kWfDiagSteps + 2 * kDiagStepBins + any]);
        for (int b = 0; b < kDiagStepBins; ++b)
            if (h[kWfDiagSteps + kDiagStepBins * any + b]) fprintf(stderr, " %d:%u", b, h[kWfDiagSteps + kDiagStepBins * any + b]);
        fprintf(stderr, "\n");
    }
}

// Whether the HIP runtime takes timeline events inside a captured frame (external event-record
// nodes).  The system ROCm 7.2 runtime the C host links does; the HIP runtime PyTorch bundles
// refuses them (hipEventRecordWithFlags(..., hipEventRecordExternal) during capture: invalid
// argument), so after the first refusal frames are captured without them: the graphs then hold
// the frame's launches, memsets and copies only, and the per-stage times of replayed frames are
// not recorded (rt_stats kernel_ms; the frame's own time, taken outside the graphs, is).
// Process-wide and one-way (true -> false) for g_graph_events; g_ext_refused is the refusal flag of a
// capture attempt.  Atomics: contexts on other threads may capture concurrently (ThreadLocal capture).
std::atomic<bool> g_graph_events{true};
thread_local bool g_ext_refused = false;   // set when this thread's capture had an external event record refused

struct Enqueue {
    WfTimeline& T;
    hipStream_t stream;
    bool capture;   // recording into a HIP graph: events and cross-stream waits are external nodes
    int last = -1;
    bool mark(const char** err) {
        if (capture && !g_graph_events) return true;   // untimed capture
        if (T.n_ev >= WfTimeline::kMaxEv) {
            *err = "wavefront timeline: too many events";
            return false;
        }
        if (!hip_ok(hipEventRecordWithFlags(T.ev[T.n_ev], stream, capture ? hipEventRecordExternal : 0u),
                    capture ? "hipEventRecordWithFlags(external)" : "hipEventRecordWithFlags(0)", err)) {
            if (capture) g_ext_refused = true;
            return false;
        }
        last = T.n_ev++;
        return true;
    }
    // closes the span [previous mark, now) as `stage`; without a previous mark (part 0 was captured
    // untimed and this part is recorded eagerly) it only marks: there is no start event to time from
    bool span(int stage, const char** err) {
        if (capture && !g_graph_events) return true;
        const int a = last;
        if (!mark(err)) return false;
        if (a >= 0) T.spans[T.n_spans++] = WfTimeline::Span{stage, a, last};
        return true;
    }
};

// One bulk round's launch geometry: the wf_trace and wf_shade grids, the input queue, and the
// device-clock span slots of the two traversal launches (-1: none)
struct Round {
    unsigned trace_grid, shade_grid;
    int cur, ts_extend, ts_connect;
};

// One frame's launch context, shared by the host-driven and the device-driven rounds.
struct Frame {
    const DevScene& S;
    WfParams& Q;
    const WfKernels& K;
    bool count, full;
    int max_bounces, maxExtra;
    bool with_extra;      // device-driven rounds: the extra-sample pass is enqueued
    hipStream_t stream;
    WfTimeline* T;        // device-driven rounds only
    const char** err;

    unsigned pixel_grid() const { return grid_for(Q.own_pixels, 1u << 30); }
    // the bulk traversal launches: Q.trace_frac percent of the resident grid, a multiple of 8 (XCDs)
    unsigned trace_grid_cap() const {
        return std::max(8u, K.trace_resident * (unsigned)std::max(Q.trace_frac, 1) / 100u / 8u * 8u);
    }

    // a launch of `grid` blocks of kBlock threads with the arguments every kernel but the sort's takes first
    template <typename Kernel, typename... Args>
    bool launch(Kernel kernel, unsigned grid, Args... args) {
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), 0, stream, S, Q.Pd, Q, args...);
        return hip_ok(hipGetLastError(), "hipGetLastError()", err);
    }

    // The launches of one bulk round: extend, the hit sort, shade, connect.  after(stage) is called
    // behind each stage's launches (stage_ms index: 1 extend, 6 sort -- also when the round has no
    // sort --, 2 shade, 3 connect) and returns false to stop.
    template <typename After>
    bool launch_round(const Round& r, After&& after) {
        const dim3 gt(r.trace_grid), g(r.shade_grid), block(kBlock);
        hipLaunchKernelGGL(K.extend, gt, block, 0, stream, S, Q.Pd, Q, r.cur, r.ts_extend);
        if (!after(1)) return false;
        if (Q.sort_bins) {
            hipLaunchKernelGGL(K.sort_hist, dim3(kSortBlocks), dim3(kSortThreads), 0, stream, S, Q, r.cur);
            hipLaunchKernelGGL(K.sort_rowscan, dim3(Q.sort_bins), dim3(kSortBlocks), 0, stream, Q);
            hipLaunchKernelGGL(K.sort_scatter, dim3(kSortBlocks), dim3(kSortThreads), 0, stream, S, Q, r.cur);
        }
        if (!after(6)) return false;
        hipLaunchKernelGGL(K.shade, g, block, 0, stream, S, Q.Pd, Q, r.cur);
        if (!after(2)) return false;
        hipLaunchKernelGGL(K.connect, gt, block, 0, stream, S, Q.Pd, Q, r.cur, r.ts_connect);
        WF_CHECK(hipGetLastError());
        return after(3);
    }

    // The finish launch: Q.finish_frac percent of the resident grid of its instance (frames in
    // flight: the rest of the machine stays free for the other frames' kernels), at least one block
    // per XCD: each takes the chunks of its XCD's counter (wf_finish_step).
    bool launch_finish(int cur, uint32_t n, int ts) {
        const unsigned cap = std::max(8u, K.finish_resident * (unsigned)Q.finish_frac / 100u);
        return launch(K.finish, std::max(8u, grid_for(n, cap)), cur, ts);
    }

    // ---- host-driven rounds: every round's queue size is read back before the next launch ----------
    bool read_counts() {
        WF_CHECK(hipMemcpyAsync(Q.W.h_counts, Q.W.counts, kWfCountWords * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        WF_CHECK(hipStreamSynchronize(stream));
        return true;
    }

    bool host_finish(int it, int cur, uint32_t n, WfFrameStats* fs) {   // the rest of the pass in one persistent launch
        WavefrontBuffers& W = Q.W;
        WF_CHECK(hipEventRecord(W.ev[0], stream));
        WF_CHECK(hipMemsetAsync(W.counts + cslot(kCntChunkFinish), 0, cslot(kShards) * sizeof(uint32_t), stream));
        if (Q.diag) {
            WF_CHECK(hipMemsetAsync(W.counts + kWfDiagHist, 0, kDiagTimeBins * sizeof(uint32_t), stream));
            WF_CHECK(hipMemsetAsync(W.counts + kWfDiagExh, 0, kDiagTimeBins * sizeof(uint32_t), stream));
            WF_CHECK(hipMemsetAsync(W.counts + kWfStat + kStatDiagShadeT, 0, kStatDiagWords * sizeof(uint32_t),
                                    stream));
        }
        if (!launch_finish(cur, n, -1)) return false;
        WF_CHECK(hipEventRecord(W.ev[1], stream));
        if (!read_counts()) return false;
        float a = 0;
        WF_CHECK(hipEventElapsedTime(&a, W.ev[0], W.ev[1]));
        fs->stage_ms[5] += a;
        ++fs->finish_launches;
        ++fs->iterations;
        if (Q.diag) print_finish_diag(W.h_counts, it, n, a);
        return true;
    }

    bool iterate(int& cur, uint32_t n, WfFrameStats* fs) {
        const int max_it = max_bounces * (max_bounces + 1) + 2;
        WavefrontBuffers& W = Q.W;
        for (int it = 0; it < max_it && n > 0; ++it) {
            if (n < Q.tail) return host_finish(it, cur, n, fs);
            WF_CHECK(hipEventRecord(W.ev[0], stream));
            // W.ev[0] extend ev[1] sort ev[4] shade ev[2] connect ev[3]
            auto after = [&](int stage) { return hip_ok(hipEventRecord(W.ev[stage == 6 ? 4 : stage], stream), "hipEventRecord", err); };
            if (!launch_round(Round{grid_for(n, trace_grid_cap()), grid_for(n, Q.shade_blocks), cur, -1, -1}, after)) return false;
            if (!read_counts()) return false;
            float ms[4] = {0, 0, 0, 0};   // extend, sort, shade, connect
            const int ev[5] = {0, 1, 4, 2, 3}, stage[4] = {1, 6, 2, 3};
            for (int i = 0; i < 4; ++i) {
                WF_CHECK(hipEventElapsedTime(&ms[i], W.ev[ev[i]], W.ev[ev[i + 1]]));
                fs->stage_ms[stage[i]] += ms[i];
            }
            fs->trace_rays += (unsigned long long)n + queue_total(W.h_counts, 2);  // extend + connect rays
            fs->trace_closest_rays += n;
            fs->trace_launches += 2;
            fs->trace_ms += ms[0] + ms[3];
            if (Q.diag) {
                print_round_diag(W.h_counts, it, n, ms, count);
                if (count) WF_CHECK(hipMemsetAsync(W.counts + kWfDiagSteps, 0, kDiagStepsWords * sizeof(uint32_t), stream));
            }
            n = queue_total(W.h_counts, 1 - cur);
            cur = 1 - cur;
            ++fs->iterations;
        }
        return true;
    }

    // ---- device-side control: the whole frame enqueued without host round trips --------------------
    // The host enqueues `rounds_for(paths)` bulk rounds per pass (enough for the live paths to fall
    // below the finish threshold when about half of them end per round), then one finish launch;
    // the extend launch of a round that finds fewer than `tail` live paths flags tail mode and
    // names its queue as the finish input, and every later bulk launch of the pass returns at once.
    // Per-stage times come from events between the launches, ray counts and rounds from device
    // counters; both are collected by wavefront_collect once the frame has finished.
    bool enqueue_pass(int rounds, int ts, Enqueue& E) {
        if (!Q.spans) ts = -1;   // no device-clock spans: the kernels skip the stamps
        auto after = [&](int stage) { return (stage == 6 && !Q.sort_bins) || E.span(stage, err); };   // no sort, no sort span
        for (int k = 0; k < rounds; ++k)
            if (!launch_round(Round{trace_grid_cap(), Q.shade_blocks, k & 1, ts + 2 * k, ts + 2 * k + 1}, after)) return false;
        // the finish chunk counter is zero here: the frame start clears every counter and the
        // extra-sample pass clears it again before its own finish launch
        if (!launch_finish(-1, 1u << 30, ts + kTsFinish)) return false;   // resident grid; input queue from the counters
        return E.span(5, err);
    }

    // One frame on `stream` in two parts: record_base = the base pass and the motion vectors,
    // record_rest = the extra-sample pass and the resolve, which read the previous frame's outputs
    // (the caller enqueues the wait for it in between).  Launch arguments come from S, Q and the
    // buffer pointers in the frame's parameters; their per-frame values are read by the kernels from Q.Pd.
    bool record_base(bool capture) {
        WavefrontBuffers& W = Q.W;
        Enqueue E{*T, stream, capture};
        T->n_ev = T->n_spans = 0;
        if (!E.mark(err)) return false;
        // counters, and the launch-span stamps when they are recorded
        T->dev_spans = Q.spans != 0;
        WF_CHECK(hipMemsetAsync(W.counts, 0, Q.spans ? kWfCountAllocBytes : kWfTsOffset, stream));
        const int rounds = rounds_for(Q.base_paths, Q.tail);
        Q.finish_q = rounds & 1;
        if (!launch(K.generate, grid_for(Q.base_paths, 16384))) return false;
        if (!E.span(0, err)) return false;
        if (!enqueue_pass(rounds, 0, E)) return false;
        if (!launch(K.motion, pixel_grid())) return false;
        return E.span(4, err);
    }

    bool record_rest(bool capture) {
        WavefrontBuffers& W = Q.W;
        Enqueue E{*T, stream, capture};
        E.last = T->n_ev - 1;   // spans continue from record_base's last event
        if (with_extra) {
            // second pass over the motion-adaptive extra samples (:779-789), appended to queue 0
            const int rounds2 = rounds_for((uint64_t)Q.own_pixels * (uint64_t)maxExtra, Q.tail);
            WF_CHECK(hipMemsetAsync(W.counts, 0, cslot(kShards) * sizeof(uint32_t), stream));
            WF_CHECK(hipMemsetAsync(W.counts + cslot(kCntBack), 0, cslot(kShards) * sizeof(uint32_t), stream));
            WF_CHECK(hipMemsetAsync(W.counts + cslot(kCntChunkExtend), 0, cslot(2 * kShards) * sizeof(uint32_t), stream));
            WF_CHECK(hipMemsetD32Async(W.counts + cslot(kCntTailMode), 0u, 1, stream));
            WF_CHECK(hipMemsetD32Async(W.counts + cslot(kCntFinishQ), (uint32_t)(rounds2 & 1), 1, stream));
            WF_CHECK(hipMemsetAsync(W.counts + cslot(kCntChunkFinish), 0, cslot(kShards) * sizeof(uint32_t), stream));
            if (!launch(K.extra, pixel_grid(), 0)) return false;
            if (!E.span(4, err)) return false;
            if (!enqueue_pass(rounds2, kTsPass, E)) return false;
        }
        if (!launch(K.resolve, pixel_grid(), with_extra ? 1 : 0)) return false;
        if (!E.span(4, err)) return false;
        WF_CHECK(hipMemcpyAsync(W.h_counts, W.counts, Q.spans ? kWfCountAllocBytes : kWfTsOffset, hipMemcpyDeviceToHost,
                                stream));
        return true;
    }

    // part `part` of the frame, eagerly or captured into T->exec[part] and launched
    bool capture_part(int part, bool rebuild) {
        if (rebuild) {
            const char* rerr = nullptr;
            Frame cap = *this;   // a refused capture is reported below, not as the frame's error
            cap.err = &rerr;
            hipGraph_t g = nullptr;
            const int n_ev = T->n_ev, n_spans = T->n_spans;
            hipError_t be, ce, ie;
            bool ok;
            for (int attempt = 0;; ++attempt) {
                g_ext_refused = false;
                be = hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal);
                ok = be == hipSuccess && (part == 0 ? cap.record_base(true) : cap.record_rest(true));
                ce = be == hipSuccess ? hipStreamEndCapture(stream, &g) : be;
                ie = hipErrorUnknown;
                if (ok && ce == hipSuccess && g) ie = hipGraphInstantiateWithFlags(&T->exec[part], g, 0);
                if (g) (void)hipGraphDestroy(g);
                g = nullptr;
                if (!ok && g_ext_refused && g_graph_events && attempt == 0) {
                    // this runtime takes no timeline events in a graph: capture untimed from now on
                    (void)hipGetLastError();
                    g_graph_events = false;
                    T->n_ev = n_ev;
                    T->n_spans = n_spans;
                    continue;
                }
                break;
            }
            if (!ok || ce != hipSuccess || ie != hipSuccess) {
                // capture refused (an API the runtime cannot capture): this slot renders eagerly from now on
                // (rt_stats total_graph_fallbacks counts its frames; the first refusal is reported here)
                static bool reported = false;
                if (!reported) {
                    reported = true;
                    fprintf(stderr, "rt: frame graph capture (part %d) refused: begin %s, record %s, end %s, instantiate %s; "
                            "the slot renders eagerly\n", part, hipGetErrorString(be), ok ? "ok" : (rerr ? rerr : "?"),
                            hipGetErrorString(ce), hipGetErrorString(ie));
                }
                (void)hipGetLastError();
                T->exec[part] = nullptr;
                T->graph_failed = true;
                T->n_ev = n_ev;
                T->n_spans = n_spans;
                return part == 0 ? record_base(false) : record_rest(false);
            }
        }
        WF_CHECK(hipGraphLaunch(T->exec[part], stream));
        return true;
    }

    bool enqueue_frame(hipEvent_t prev_done, bool graphs) {
        Q.dev_ctl = 1;   // Q.finish_q: set by record_base from the round count
        const bool eager = !graphs || T->graph_failed;   // graphs off, or a capture of this slot was refused before
        // The frame's launches, memsets and copies only take S, Q (by value) and the slot's fixed
        // buffers and events; everything that changes per frame is in the device FrameParams, uploaded
        // before the launch.  So the graph is valid while these bytes are.
        std::vector<uint8_t> key(eager ? 0 : sizeof(DevScene) + sizeof(WfParams) + 4 * sizeof(int));
        bool rebuild = false;
        if (!eager) {
            WfParams Qk = Q;
            Qk.W.param_slot = 0;   // the upload ring position is host bookkeeping
            uint8_t* k = key.data();
            std::memcpy(k, &S, sizeof S);
            std::memcpy(k + sizeof S, &Qk, sizeof Qk);
            const int flags[4] = {count ? 1 : 0, full ? 1 : 0, with_extra ? 1 : 0, maxExtra};
            std::memcpy(k + sizeof S + sizeof Qk, flags, sizeof flags);
            rebuild = !T->exec[0] || !T->exec[1] || T->key != key;
        }
        if (rebuild) {
            // the slot's previous frame has finished (its slot was harvested): its graphs can go
            for (hipGraphExec_t& x : T->exec)
                if (x) {
                    WF_CHECK(hipGraphExecDestroy(x));
                    x = nullptr;
                }
            T->key.clear();
        }
        if (!(eager ? record_base(false) : capture_part(0, rebuild))) return false;
        if (prev_done) WF_CHECK(hipStreamWaitEvent(stream, prev_done, 0));
        // graph_failed: set by capture_part when part 0 could not be captured
        if (!(eager || T->graph_failed ? record_rest(false) : capture_part(1, rebuild))) return false;
        if (rebuild && !T->graph_failed) T->key.swap(key);
        T->graph_mode = !graphs ? kGraphEager : T->graph_failed ? kGraphFallback : rebuild ? kGraphCapture : kGraphReplay;
        T->pending = true;
        return true;
    }

    // host-driven rounds: the whole frame, finished when it returns
    bool run_host_rounds(hipEvent_t prev_done, WfFrameStats* fs) {
        WavefrontBuffers& W = Q.W;
        WF_CHECK(hipEventRecord(W.ev[0], stream));
        WF_CHECK(hipMemsetAsync(W.counts, 0, kWfCountWords * sizeof(uint32_t), stream));
        if (!launch(K.generate, grid_for(Q.base_paths, 16384))) return false;
        WF_CHECK(hipEventRecord(W.ev[1], stream));
        if (!read_counts()) return false;
        float ms = 0;
        WF_CHECK(hipEventElapsedTime(&ms, W.ev[0], W.ev[1]));
        fs->stage_ms[0] += ms;
        int cur = 0;
        if (!iterate(cur, queue_total(W.h_counts, 0), fs)) return false;

        if (prev_done) WF_CHECK(hipStreamWaitEvent(stream, prev_done, 0));
        WF_CHECK(hipEventRecord(W.ev[0], stream));
        if (!launch(K.motion, pixel_grid())) return false;
        if (maxExtra > 0) {
            // the extra-sample pass appends primary rays to queue `cur` (reset here)
            WF_CHECK(hipMemsetAsync(W.counts + cslot(cur * kShards), 0, cslot(kShards) * sizeof(uint32_t), stream));
            WF_CHECK(hipMemsetAsync(W.counts + cslot(kCntBack + cur * kShards), 0, cslot(kShards) * sizeof(uint32_t), stream));
            if (!launch(K.extra, pixel_grid(), cur)) return false;
            if (!read_counts()) return false;
            const uint32_t n_extra = queue_total(W.h_counts, cur);
            if (n_extra > 0 && !iterate(cur, n_extra, fs)) return false;
        }
        if (!launch(K.resolve, pixel_grid(), maxExtra > 0 ? 1 : 0)) return false;
        WF_CHECK(hipEventRecord(W.ev[1], stream));
        WF_CHECK(hipStreamSynchronize(stream));
        WF_CHECK(hipEventElapsedTime(&ms, W.ev[0], W.ev[1]));
        fs->stage_ms[4] += ms;
        return true;
    }
};

}  // namespace

bool wavefront_collect(const WavefrontBuffers& W, WfTimeline& T, WfFrameStats* fs, const char** err) {
    if (!T.pending) return true;
    T.pending = false;
    *fs = WfFrameStats{};
    for (int i = 0; i < T.n_spans; ++i) {
        const WfTimeline::Span& sp = T.spans[i];
        float ms = 0.0f;
        WF_CHECK(hipEventElapsedTime(&ms, T.ev[sp.a], T.ev[sp.b]));
        fs->stage_ms[sp.stage] += ms;
        if (sp.stage == 1 || sp.stage == 3) fs->trace_ms += ms;
    }
    fs->iterations = (int)W.h_counts[kWfStat + kStatRounds];
    fs->trace_launches = (int)W.h_counts[kWfStat + kStatTraceLaunches];
    fs->trace_rays = W.h_counts[kWfStat + kStatTraceRays];
    fs->trace_closest_rays = W.h_counts[kWfStat + kStatExtendRays];
    fs->finish_launches = (int)W.h_counts[kWfStat + kStatFinish];
    fs->graph_mode = T.graph_mode;
    for (int pass = 0; pass < (T.dev_spans ? 2 : 0); ++pass)   // device-clock spans (10 ns ticks) of the launches that ran
        for (int k = 0; k <= kTsFinish; ++k) {
            const int slot = pass * kTsPass + k;
            const unsigned long long a = W.h_tstamp[slot * kTsStride];
            unsigned long long b = 0;
            for (int x = 1; x <= kTsXcds; ++x) b = std::max(b, W.h_tstamp[slot * kTsStride + kTsLine * x]);
            if (a == 0 || b <= a) continue;
            const float ms = (float)((double)(b - a) * 1e-5);
            if (k == kTsFinish) {
                fs->finish_dev_ms += ms;
                fs->finish_dev_launches++;
            } else if (k < 2 * kTsRounds) {
                fs->trace_dev_ms += ms;
                fs->trace_dev_launches++;
            }
        }
    return true;
}

bool run_wavefront(const DevScene& S, const FrameParams& P, WavefrontBuffers& W, const WfTuning& tu,
                   const WfSchedule& sched, int own_tiles, bool count, bool spans, int sort_bins, bool extra_pass,
                   hipStream_t stream, hipEvent_t prev_done, WfTimeline* tl, WfFrameStats* fs, const char** err,
                   bool graphs) {
    WfParams Q;
    std::memset(&Q, 0, sizeof Q);   // no stray padding bytes (frame-graph key)
    Q.W = W;
    Q.spp = max(P.U.samplesPerPixel, 1);
    Q.own_pixels = (uint32_t)own_tiles * (uint32_t)P.tile_size * (uint32_t)P.tile_size;
    Q.base_paths = Q.own_pixels * (uint32_t)Q.spp;
    Q.seg_cap = (uint32_t)(W.queue_entries / kShards);
    Q.refill_min = tu.refill_min;
    Q.chunk = tu.chunk;
    Q.tail = sched.tail;
    Q.sort_bins = (uint32_t)sort_bins;
    Q.diag = tu.log;
    Q.shade_min = tu.shade_min;
    Q.shade_min_x = tu.shade_min_x;
    Q.team = sched.team;
    Q.fchunk = tu.fchunk;
    Q.shade_blocks = tu.shade_blocks;
    Q.spans = spans ? 1 : 0;
    Q.count = count ? 1 : 0;
    Q.px.spp_div = make_fastdiv((uint32_t)Q.spp);
    Q.px.tile = P.tile_size;
    Q.px.rank = P.rank;
    Q.px.nranks = P.nranks;
    Q.px.tile_px_div = make_fastdiv((uint32_t)P.tile_size * (uint32_t)P.tile_size);
    Q.px.tiles_x_div = make_fastdiv((uint32_t)max(P.tiles_x, 1));
    Q.trace_frac = sched.trace_frac;
    Q.finish_frac = sched.finish_frac;
    if (sort_bins && (sort_bins < kSortMinBins || sort_bins > kSortMaxBins || (sort_bins & (sort_bins - 1)) ||
                      !S.tri_bin || !W.sorted)) {
        *err = "bad hit-sort configuration";
        return false;
    }
    *fs = WfFrameStats{};
    // tail <= 1 (bulk rounds only, a test configuration) keeps the host loop: its round count is
    // only bounded by maxBounces * (maxBounces + 1)
    const bool dev = tl && !tu.host_ctl && !tu.log && Q.tail > 1;
    Q.Pd = W.d_params;
    {   // this frame's parameters -> device; the slot's previous upload has executed once its event has
        const int slot = W.param_slot;
        W.param_slot = (slot + 1) % WavefrontBuffers::kParamSlots;
        WF_CHECK(hipEventSynchronize(W.param_ev[slot]));
        W.h_params[slot] = P;
        WF_CHECK(hipMemcpyAsync(W.d_params, &W.h_params[slot], sizeof(FrameParams), hipMemcpyHostToDevice, stream));
        WF_CHECK(hipEventRecord(W.param_ev[slot], stream));
    }
    const bool full = needs_full(P.U, S);
    const int maxExtra = (P.U.enableMotionAdaptiveSampling != 0) ? max(P.U.motionSamplingMaxExtraSamples, 0) : 0;
    // wf_kernels' first call makes the device queries behind the grid sizes: here, before a stream is capturing
    Frame F{S, Q, wf_kernels(count, full, sort_bins != 0, Q.team != 0), count, full, P.U.maxBounces, maxExtra,
            maxExtra > 0 && extra_pass, stream, tl, err};
    return dev ? F.enqueue_frame(prev_done, graphs) : F.run_host_rounds(prev_done, fs);
}

}  // namespace rt
