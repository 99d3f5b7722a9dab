"""The frame ring (csrc/rt_frame_ring.h): which slot a frame takes, what it waits for, the
geometry generations and the motion targets, as pure host functions.  tools/frame_ring_print.cpp is
compiled with plain g++ (the header includes no HIP header; with the address and undefined-
behaviour sanitizers where they link) and driven by scripts.

(a) Scripted sequences against a literal table, worked out by hand from the rules as they stood
in rt_render_frame, begin_update, tiles_op and rt_resize before they moved into the header:
  slot        = first frame since rt_resize ? 0 : (last slot + 1) % nfl
  cross       = not the first frame, and the last slot is used, and (last slot != slot or a pack /
                unpack followed the last frame)
  retile_wait = a pack / unpack followed the last frame, and the tile set differs from that
                frame's, and the last slot is used
  ctx_wait    = slot != 0 and the slot has not waited for the newest work on the context's stream
  flip        = an update since the last frame; then gen = (gcur + 1) % ngens (the old ngens)
  drain       = nfl differs from the last frame's, which exists; then ngens = max(2, nfl, gen + 1)
  motion      = wavefront: reads m, writes (m + 1) % 9; megakernel: m in place
  update      = the first since a frame writes (gcur + 1) % ngens after waiting for the used slots
                whose frame reads that generation; the following ones write there too
  resize      = no slot used, frame count, last slot, motion and accumulation index 0; the rest stays
(b) A hazard check over the same sequences and seeded random ones.  A frame counts as finished
only once the host has waited for it: its slot is harvested for the next frame, a drain, rt_wait,
or the wait an update orders.  No update may write a generation an unfinished frame reads, and no
frame may write a motion target an unfinished frame reads or writes."""
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# F: (slot, cross, retile_wait, ctx_wait, flip, drain, ngens, gen, motion_prev, motion_out)
# U: (seed, dst, wait mask)      T: (newest slot used,)      C: (ctx_work,)      W: used slots, oldest first
W4, W2, W8, W1, MEGA = "F 4 1 64 0 1", "F 2 1 64 0 1", "F 8 1 64 0 1", "F 1 1 64 0 1", "F 1 0 64 0 1"
SEQUENCES = {
    # first frame, steady rotation over four slots, the motion targets wrapping at nine
    "steady4": [
        (W4, (0, 0, 0, 0, 0, 0, 4, 0, 0, 1)), (W4, (1, 1, 0, 1, 0, 0, 4, 0, 1, 2)),
        (W4, (2, 1, 0, 1, 0, 0, 4, 0, 2, 3)), (W4, (3, 1, 0, 1, 0, 0, 4, 0, 3, 4)),
        (W4, (0, 1, 0, 0, 0, 0, 4, 0, 4, 5)), (W4, (1, 1, 0, 0, 0, 0, 4, 0, 5, 6)),
        (W4, (2, 1, 0, 0, 0, 0, 4, 0, 6, 7)), (W4, (3, 1, 0, 0, 0, 0, 4, 0, 7, 8)),
        (W4, (0, 1, 0, 0, 0, 0, 4, 0, 8, 0)), (W4, (1, 1, 0, 0, 0, 0, 4, 0, 0, 1)),
        ("W", (2, 3, 0, 1)),
    ],
    "steady1": [
        ("W", ()),
        (W1, (0, 0, 0, 0, 0, 0, 2, 0, 0, 1)), (W1, (0, 0, 0, 0, 0, 0, 2, 0, 1, 2)),
        (W1, (0, 0, 0, 0, 0, 0, 2, 0, 2, 3)), ("W", (0,)),
    ],
    "steady2": [
        (W2, (0, 0, 0, 0, 0, 0, 2, 0, 0, 1)), (W2, (1, 1, 0, 1, 0, 0, 2, 0, 1, 2)),
        (W2, (0, 1, 0, 0, 0, 0, 2, 0, 2, 3)), (W2, (1, 1, 0, 0, 0, 0, 2, 0, 3, 4)),
    ],
    "steady8": [
        (W8, (0, 0, 0, 0, 0, 0, 8, 0, 0, 1)), (W8, (1, 1, 0, 1, 0, 0, 8, 0, 1, 2)),
        (W8, (2, 1, 0, 1, 0, 0, 8, 0, 2, 3)), (W8, (3, 1, 0, 1, 0, 0, 8, 0, 3, 4)),
        (W8, (4, 1, 0, 1, 0, 0, 8, 0, 4, 5)), (W8, (5, 1, 0, 1, 0, 0, 8, 0, 5, 6)),
        (W8, (6, 1, 0, 1, 0, 0, 8, 0, 6, 7)), (W8, (7, 1, 0, 1, 0, 0, 8, 0, 7, 8)),
        (W8, (0, 1, 0, 0, 0, 0, 8, 0, 8, 0)), (W8, (1, 1, 0, 0, 0, 0, 8, 0, 0, 1)),
        ("W", (2, 3, 4, 5, 6, 7, 0, 1)),
    ],
    # megakernel frames: one slot, the motion target in place; then a wavefront frame on one slot
    "megakernel": [
        (MEGA, (0, 0, 0, 0, 0, 0, 2, 0, 0, 0)), (MEGA, (0, 0, 0, 0, 0, 0, 2, 0, 0, 0)),
        (W1, (0, 0, 0, 0, 0, 0, 2, 0, 0, 1)), (MEGA, (0, 0, 0, 0, 0, 0, 2, 0, 1, 1)),
    ],
    # an update before every frame: a generation flip each frame, the fifth update waits for slot 0
    "update_every_frame": [
        ("U", (1, 1, 0)), (W4, (0, 0, 0, 0, 1, 0, 4, 1, 0, 1)),
        ("U", (1, 2, 0)), (W4, (1, 1, 0, 1, 1, 0, 4, 2, 1, 2)),
        ("U", (1, 3, 0)), (W4, (2, 1, 0, 1, 1, 0, 4, 3, 2, 3)),
        ("U", (1, 0, 0)), (W4, (3, 1, 0, 1, 1, 0, 4, 0, 3, 4)),
        ("U", (1, 1, 1)), (W4, (0, 1, 0, 0, 1, 0, 4, 1, 4, 5)),
        ("U", (1, 2, 2)), ("U", (0, 2, 0)), (W4, (1, 1, 0, 0, 1, 0, 4, 2, 5, 6)),
    ],
    "update_now_and_then": [
        (W2, (0, 0, 0, 0, 0, 0, 2, 0, 0, 1)), (W2, (1, 1, 0, 1, 0, 0, 2, 0, 1, 2)),
        ("U", (1, 1, 0)), (W2, (0, 1, 0, 0, 1, 0, 2, 1, 2, 3)), (W2, (1, 1, 0, 0, 0, 0, 2, 1, 3, 4)),
        ("U", (1, 0, 0)), (W2, (0, 1, 0, 0, 1, 0, 2, 0, 4, 5)),
        ("U", (1, 1, 2)), (W2, (1, 1, 0, 0, 1, 0, 2, 1, 5, 6)),
        ("U", (1, 0, 1)),
    ],
    # frames in flight 4 -> 2 -> 8 while gcur is 0: a drain each time, ngens follows nfl
    "nfl_change_gen0": [
        (W4, (0, 0, 0, 0, 0, 0, 4, 0, 0, 1)), (W4, (1, 1, 0, 1, 0, 0, 4, 0, 1, 2)),
        (W4, (2, 1, 0, 1, 0, 0, 4, 0, 2, 3)),
        (W2, (1, 1, 0, 0, 0, 1, 2, 0, 3, 4)), (W8, (2, 1, 0, 0, 0, 1, 8, 0, 4, 5)),
    ],
    # ... while gcur is the highest generation: ngens >= gcur + 1 keeps four; then the flip to 0 and eight
    "nfl_change_gen_top": [
        ("U", (1, 1, 0)), (W4, (0, 0, 0, 0, 1, 0, 4, 1, 0, 1)),
        ("U", (1, 2, 0)), (W4, (1, 1, 0, 1, 1, 0, 4, 2, 1, 2)),
        ("U", (1, 3, 0)), (W4, (2, 1, 0, 1, 1, 0, 4, 3, 2, 3)),
        (W2, (1, 1, 0, 0, 0, 1, 4, 3, 3, 4)),
        ("U", (1, 0, 0)), (W8, (2, 1, 0, 0, 1, 1, 8, 0, 4, 5)),
    ],
    # ... and the flip into the highest generation in the frame that changes the frames in flight
    "nfl_change_flip_top": [
        ("U", (1, 1, 0)), (W4, (0, 0, 0, 0, 1, 0, 4, 1, 0, 1)),
        ("U", (1, 2, 0)), (W4, (1, 1, 0, 1, 1, 0, 4, 2, 1, 2)),
        ("U", (1, 3, 0)), (W2, (0, 1, 0, 0, 1, 1, 4, 3, 2, 3)),
    ],
    # a pack on the context's stream, then the same tile set (no wait for it), then another one
    "pack_four_slots": [
        ("F 4 1 64 1 2", (0, 0, 0, 0, 0, 0, 4, 0, 0, 1)), ("T 1", (1,)),
        ("F 4 1 64 1 2", (1, 1, 0, 1, 0, 0, 4, 0, 1, 2)), ("T 1", (1,)),
        ("F 4 1 64 0 2", (2, 1, 1, 1, 0, 0, 4, 0, 2, 3)),
        ("F 4 1 64 1 2", (3, 1, 0, 1, 0, 0, 4, 0, 3, 4)),
        ("F 4 1 64 1 2", (0, 1, 0, 0, 0, 0, 4, 0, 4, 5)),
        ("F 4 1 64 1 2", (1, 1, 0, 1, 0, 0, 4, 0, 5, 6)),
    ],
    # one slot, packs on a caller's stream: the next frame of the same slot must follow the pack
    "pack_one_slot": [
        ("F 1 1 32 0 1", (0, 0, 0, 0, 0, 0, 2, 0, 0, 1)), ("T 0", (1,)),
        ("F 1 1 32 0 1", (0, 1, 0, 0, 0, 0, 2, 0, 1, 2)),
        ("F 1 1 32 0 1", (0, 0, 0, 0, 0, 0, 2, 0, 2, 3)), ("T 0", (1,)),
        ("F 1 1 32 0 2", (0, 1, 1, 0, 0, 0, 2, 0, 3, 4)),
    ],
    "pack_before_first_frame": [
        ("T 1", (0,)), (W2, (0, 0, 0, 0, 0, 0, 2, 0, 0, 1)), (W2, (1, 1, 0, 1, 0, 0, 2, 0, 1, 2)),
    ],
    # work on the context's stream between frames: only the slots that have not seen it wait
    "ctx_work": [
        (W4, (0, 0, 0, 0, 0, 0, 4, 0, 0, 1)), (W4, (1, 1, 0, 1, 0, 0, 4, 0, 1, 2)),
        (W4, (2, 1, 0, 1, 0, 0, 4, 0, 2, 3)), ("C", (2,)),
        (W4, (3, 1, 0, 1, 0, 0, 4, 0, 3, 4)), (W4, (0, 1, 0, 0, 0, 0, 4, 0, 4, 5)),
        (W4, (1, 1, 0, 1, 0, 0, 4, 0, 5, 6)), (W4, (2, 1, 0, 1, 0, 0, 4, 0, 6, 7)),
        (W4, (3, 1, 0, 0, 0, 0, 4, 0, 7, 8)), (W4, (0, 1, 0, 0, 0, 0, 4, 0, 8, 0)),
        (W4, (1, 1, 0, 0, 0, 0, 4, 0, 0, 1)),
    ],
    # a resize (three pieces of work on the context's stream, then the reset) in mid sequence: slot
    # and motion start over, generation and rotation stay, stale slots are not waited for
    "resize": [
        ("U", (1, 1, 0)), (W4, (0, 0, 0, 0, 1, 0, 4, 1, 0, 1)), (W4, (1, 1, 0, 1, 0, 0, 4, 1, 1, 2)),
        (W4, (2, 1, 0, 1, 0, 0, 4, 1, 2, 3)),
        ("C", (2,)), ("C", (3,)), ("C", (4,)), ("R", ()), ("W", ()),
        (W4, (0, 0, 0, 0, 0, 0, 4, 1, 0, 1)), (W4, (1, 1, 0, 1, 0, 0, 4, 1, 1, 2)),
        ("U", (1, 2, 0)), (W4, (2, 1, 0, 1, 1, 0, 4, 2, 2, 3)),
        ("U", (1, 3, 0)), (W4, (3, 1, 0, 1, 1, 0, 4, 3, 3, 4)),
        ("U", (1, 0, 0)), (W4, (0, 1, 0, 0, 1, 0, 4, 0, 4, 5)),
        ("U", (1, 1, 2)),
    ],
}


def build_tool(out_dir, root=ROOT):
    """tools/frame_ring_print.cpp against the header under `root`; sanitized if that links."""
    exe = os.path.join(str(out_dir), "frame_ring_print")
    cmd = ["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", root,
           os.path.join(ROOT, "tools", "frame_ring_print.cpp"), "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(cmd + san, capture_output=True).returncode != 0:
        subprocess.run(cmd, check=True)
    return exe


def run_ops(exe, ops):
    r = subprocess.run([exe], input="".join(op + "\n" for op in ops), capture_output=True, text=True, timeout=30,
                       check=True)
    out = [(line.split()[0], tuple(int(v) for v in line.split()[1:])) for line in r.stdout.splitlines()]
    assert len(out) == len(ops) and all(o[0] == op[0] for o, op in zip(out, ops))
    return [o[1] for o in out]


def check_hazards(ops, out):
    """The two rotation rules over one ring's operations and what the ring answered."""
    live = {}   # slot -> (generation read, motion target read, motion target written) of its unfinished frame
    for op, res in zip(ops, out):
        if op[0] == "F":
            slot, drain, gen, m_prev, m_out = res[0], res[5], res[7], res[8], res[9]
            live.pop(slot, None)   # harvested
            if drain:
                live.clear()
            for s, (_, r, w) in live.items():
                assert m_out not in (r, w), f"{op}: writes motion target {m_out}, slot {s}'s frame uses {r}, {w}"
            live[slot] = (gen, m_prev, m_out)
        elif op[0] == "U":
            seed, dst, mask = res
            for s in [s for s in live if mask >> s & 1]:
                del live[s]
            for s, (g, _, _) in live.items():
                assert g != dst, f"{op}: writes generation {dst}, which slot {s}'s frame reads"
        elif op[0] in "RW":   # rt_resize drains first; rt_wait harvests every slot
            live.clear()


def random_ops(seed, n=120):
    rng = random.Random(seed)
    nfl, ops = rng.choice([1, 2, 3, 4, 8]), []
    for _ in range(n):
        x = rng.random()
        if x < 0.55:
            if rng.random() < 0.06:
                nfl = rng.choice([1, 2, 3, 4, 5, 8])
            if rng.random() < 0.05:
                ops.append("F 1 0 64 0 1")   # a megakernel frame
            else:
                ops.append(f"F {nfl} 1 64 {rng.choice([0, 0, 0, 1])} 2")
        elif x < 0.85:
            ops.append("U")
        elif x < 0.91:
            ops.append(f"T {rng.randrange(2)}")
        elif x < 0.95:
            ops.append("C")
        elif x < 0.98:
            ops.append("W")
        else:
            ops.append("R")
    return ops


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    return build_tool(tmp_path_factory.mktemp("ring"))


@pytest.fixture(scope="module")
def scripted(tool):
    ops = [op for seq in SEQUENCES.values() for op in ["N"] + [o for o, _ in seq]]
    out, res = iter(run_ops(tool, ops)), {}
    for name, seq in SEQUENCES.items():
        next(out)
        res[name] = [next(out) for _ in seq]
    return res


@pytest.mark.parametrize("name", SEQUENCES)
def test_plan_table(scripted, name):
    for i, ((op, want), got) in enumerate(zip(SEQUENCES[name], scripted[name])):
        assert got == want, f"{name} step {i}: {op}"


def test_hazards(tool, scripted):
    for name, seq in SEQUENCES.items():
        check_hazards([op for op, _ in seq], scripted[name])
    seqs = [random_ops(seed) for seed in range(300)]
    out = iter(run_ops(tool, [op for ops in seqs for op in ["N"] + ops]))
    for ops in seqs:
        next(out)
        check_hazards(ops, [next(out) for _ in ops])
