// Prints the wavefront frame schedule (csrc/rt_wf_schedule.h) for every input line
//   frame_paths base_paths hw_slots requested_slots tail_requested trace_frac finish_frac team
// (the last three as in WfTuning: 0 0 -1 = by the schedule) as
//   in_flight tail trace_frac finish_frac team
// tests/test_wf_schedule.py compiles it with plain g++ and compares against a literal table.
#include <cstdio>

#include "metal4-raytracing_amd/csrc/rt_wf_schedule.h"

int main() {
    unsigned long long frame_paths, base_paths;
    int hw_slots, requested, tail_requested;
    rt::WfTuning tu;
    while (scanf("%llu %llu %d %d %d %d %d %d", &frame_paths, &base_paths, &hw_slots, &requested, &tail_requested,
                 &tu.trace_frac, &tu.finish_frac, &tu.team) == 8) {
        const int nfl = rt::wf_in_flight(frame_paths, hw_slots, requested);
        const rt::WfSchedule s = rt::wf_schedule((uint32_t)base_paths, nfl, tail_requested, tu);
        printf("%d %u %d %d %d\n", s.in_flight, s.tail, s.trace_frac, s.finish_frac, s.team);
    }
    return 0;
}
