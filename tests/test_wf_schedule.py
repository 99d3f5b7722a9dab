"""The wavefront frame schedule (csrc/rt_wf_schedule.h: frames in flight, finish threshold, grid
shares of the traversal and finish launches, team drain) as one pure host function, against a
literal table.  tools/wf_schedule_print.cpp is compiled with plain g++ (the header includes no HIP
header).  The expected values were worked out by hand from the formulae as they stood in
rt_render_frame and run_wavefront before they moved into the header, not from the header:
  slots     = requested, else max(2, min(frame < 2^19 paths ? min(4, hw) : hw, 96 GiB / (300 B * frame + 1)))
  tail      = requested, else 786432 with >= 8 slots and <= 2.5M base paths, else by slots
              (2: 1310720, 3: 1048576, 4: 786432, >= 5: 524288), one slot: WfTuning::tail = 4194304
  trace %   = >= 8 slots: 20 up to 2.5M base paths, 30 up to 6M, 40 above; >= 4 slots: 60; else 100
  finish %  = >= 8 slots and <= 6M base paths: 12; >= 4 slots: 20; 2: 40; 3: 33; 1: 100
  team      = 4 for 262144 .. 2.5M base paths, else 0
and a WfTuning trace_frac / finish_frac > 0 or team >= 0 wins."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

C3G = 30 * 17 * 4096 * 4          # 1920x1080 in 64-pixel tiles, 4 spp: 8,355,840 paths
SHARE8 = 64 * 4096 * 4            # an 8-way rank share: 1,048,576
UHD16 = 60 * 34 * 4096 * 16       # 3840x2160, 16 spp: 133,693,440

# (frame paths, base paths, hardware slots, requested slots, requested tail, tuning trace %, finish %, team)
#   -> (frames in flight, tail, trace %, finish %, team)
ROWS = [
    ((C3G, C3G, 8, 0, 0, 0, 0, -1), (8, 524288, 40, 20, 0)),
    ((C3G, C3G, 4, 0, 0, 0, 0, -1), (4, 786432, 60, 20, 0)),
    ((SHARE8, SHARE8, 8, 0, 0, 0, 0, -1), (8, 786432, 20, 12, 4)),
    ((SHARE8, SHARE8, 4, 0, 0, 0, 0, -1), (4, 786432, 60, 20, 4)),
    ((65536, 65536, 8, 0, 0, 0, 0, -1), (4, 786432, 60, 20, 0)),
    ((65536, 65536, 4, 0, 0, 0, 0, -1), (4, 786432, 60, 20, 0)),
    # the 96 GiB budget: 40 GB a slot -> two; 18 GB a slot -> five; more than the budget -> still two
    ((UHD16, UHD16, 8, 0, 0, 0, 0, -1), (2, 1310720, 100, 40, 0)),
    ((UHD16, UHD16, 4, 0, 0, 0, 0, -1), (2, 1310720, 100, 40, 0)),
    ((60000000, 60000000, 8, 0, 0, 0, 0, -1), (5, 524288, 60, 20, 0)),
    ((60000000, 60000000, 4, 0, 0, 0, 0, -1), (4, 786432, 60, 20, 0)),
    ((1000000000, 1000000000, 8, 0, 0, 0, 0, -1), (2, 1310720, 100, 40, 0)),
    # the extra samples count for the slots, not for the shares: 1 spp + 1 extra
    ((2 * 262144, 262144, 8, 0, 0, 0, 0, -1), (8, 786432, 20, 12, 4)),
    ((2 * 262143, 262143, 8, 0, 0, 0, 0, -1), (4, 786432, 60, 20, 0)),
    # requested slots win over queues, frame size and budget
    ((1000000, 1000000, 8, 1, 0, 0, 0, -1), (1, 4194304, 100, 100, 4)),
    ((1000000, 1000000, 8, 2, 0, 0, 0, -1), (2, 1310720, 100, 40, 4)),
    ((1000000, 1000000, 8, 3, 0, 0, 0, -1), (3, 1048576, 100, 33, 4)),
    ((1000000, 1000000, 4, 8, 0, 0, 0, -1), (8, 786432, 20, 12, 4)),
    ((C3G, C3G, 8, 1, 0, 0, 0, -1), (1, 4194304, 100, 100, 0)),
    ((C3G, C3G, 8, 4, 0, 0, 0, -1), (4, 786432, 60, 20, 0)),
    ((C3G, C3G, 8, 5, 0, 0, 0, -1), (5, 524288, 60, 20, 0)),
    ((C3G, C3G, 8, 7, 0, 0, 0, -1), (7, 524288, 60, 20, 0)),
    ((C3G, C3G, 8, 16, 0, 0, 0, -1), (16, 524288, 40, 20, 0)),
    ((UHD16, UHD16, 8, 8, 0, 0, 0, -1), (8, 524288, 40, 20, 0)),
    ((65536, 65536, 8, 8, 0, 0, 0, -1), (8, 786432, 20, 12, 0)),
    # a requested tail wins in every case
    ((C3G, C3G, 8, 0, 2048, 0, 0, -1), (8, 2048, 40, 20, 0)),
    ((SHARE8, SHARE8, 8, 0, 2048, 0, 0, -1), (8, 2048, 20, 12, 4)),
    ((1000000, 1000000, 8, 1, 2048, 0, 0, -1), (1, 2048, 100, 100, 4)),
    ((UHD16, UHD16, 8, 0, 2048, 0, 0, -1), (2, 2048, 100, 40, 0)),
    ((65536, 65536, 8, 0, 1, 0, 0, -1), (4, 1, 60, 20, 0)),
    # tuning overrides
    ((C3G, C3G, 8, 0, 0, 75, 0, -1), (8, 524288, 75, 20, 0)),
    ((C3G, C3G, 8, 0, 0, 0, 50, -1), (8, 524288, 40, 50, 0)),
    ((C3G, C3G, 8, 0, 0, 0, 0, 2), (8, 524288, 40, 20, 2)),
    ((SHARE8, SHARE8, 8, 0, 0, 1, 1, 0), (8, 786432, 1, 1, 0)),
    ((SHARE8, SHARE8, 8, 1, 0, 100, 100, 8), (1, 4194304, 100, 100, 8)),
    # boundaries: 2^19 frame paths (four slots below)
    ((524287, 524287, 8, 0, 0, 0, 0, -1), (4, 786432, 60, 20, 4)),
    ((524288, 524288, 8, 0, 0, 0, 0, -1), (8, 786432, 20, 12, 4)),
    ((524288, 524288, 4, 0, 0, 0, 0, -1), (4, 786432, 60, 20, 4)),
    # 2.5M base paths: tail share, trace share and team drain end together
    ((2500000, 2500000, 8, 0, 0, 0, 0, -1), (8, 786432, 20, 12, 4)),
    ((2500001, 2500001, 8, 0, 0, 0, 0, -1), (8, 524288, 30, 12, 0)),
    ((2500000, 2500000, 4, 0, 0, 0, 0, -1), (4, 786432, 60, 20, 4)),
    ((2500001, 2500001, 4, 0, 0, 0, 0, -1), (4, 786432, 60, 20, 0)),
    # 6M base paths: trace 30 -> 40 %, finish 12 -> 20 %
    ((6000000, 6000000, 8, 0, 0, 0, 0, -1), (8, 524288, 30, 12, 0)),
    ((6000001, 6000001, 8, 0, 0, 0, 0, -1), (8, 524288, 40, 20, 0)),
    # 262144 base paths: the team drain begins
    ((262143, 262143, 8, 0, 0, 0, 0, -1), (4, 786432, 60, 20, 0)),
    ((262144, 262144, 8, 0, 0, 0, 0, -1), (4, 786432, 60, 20, 4)),
    ((262143, 262143, 8, 8, 0, 0, 0, -1), (8, 786432, 20, 12, 0)),
    ((262144, 262144, 8, 8, 0, 0, 0, -1), (8, 786432, 20, 12, 4)),
]


@pytest.fixture(scope="module")
def schedules(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("wfs") / "wf_schedule_print")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", ROOT,
                    os.path.join(ROOT, "tools", "wf_schedule_print.cpp"), "-o", exe], check=True)
    stdin = "".join(" ".join(str(v) for v in inp) + "\n" for inp, _ in ROWS)
    r = subprocess.run([exe], input=stdin, capture_output=True, text=True, timeout=30, check=True)
    out = [tuple(int(v) for v in line.split()) for line in r.stdout.splitlines()]
    assert len(out) == len(ROWS)
    return out


@pytest.mark.parametrize("i", range(len(ROWS)), ids=["-".join(str(v) for v in inp) for inp, _ in ROWS])
def test_schedule_row(schedules, i):
    assert schedules[i] == ROWS[i][1], ROWS[i][0]


def test_headline_frame_sizes():
    assert (C3G, SHARE8, UHD16) == (8355840, 1048576, 133693440)
