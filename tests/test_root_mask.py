"""The root-word start of the stepwise traversal (csrc/rt_trav.h trav_start_root; csrc/rt_device.h root_word,
node8_hit_slots, node8_decode), evaluated on the host: tools/root_mask_check.cpp is compiled with plain g++
together with the BVH builder and steps seeded rays against three small BVHs whose roots are all leaves, internal
children beside leaf triangles, and eight internal children.  Every query runs from the virtual root group, from
the producer's word and from a word of 0, closest-hit and any-hit; the tool counts every disagreement (hit record
bits, node visits with the root counted, triangle tests, order of the triangle slots, steps), all of which must
be zero."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAYS = 4200   # 600 per ray class
CLASSES = ["inside", "outside", "axis", "miss", "shadow_before", "shadow_inside", "shadow_beyond"]


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("root_mask")), "root_mask_check")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off",
                    "-D__HIP_PLATFORM_AMD__", "-I", ROOT, "-I", os.path.join(rocm, "include"),
                    os.path.join(ROOT, "tools", "root_mask_check.cpp"),
                    os.path.join(ROOT, "metal4-raytracing_amd", "csrc", "rt_bvh.cpp"), "-o", exe], check=True)
    cache = {}

    def run(kind):
        """(summary fields, per-class fields) of the tool's answer for a root of `kind`."""
        if kind not in cache:
            r = subprocess.run([exe, kind, str(RAYS)], capture_output=True, text=True, timeout=120, check=True)
            lines = r.stdout.split("\n")[:-1]
            head = lines[0].split()
            assert head[0] == kind
            summary = {k: int(v) for k, v in zip(head[1::2], head[2::2])}
            classes = {}
            for line in lines[1:]:
                w = line.split()
                assert w[0] == "class"
                classes[w[1]] = {k: int(v) for k, v in zip(w[2::2], w[3::2])}
            cache[kind] = (summary, classes)
        return cache[kind]
    return run


@pytest.mark.parametrize("kind", ["leaves", "mixed", "inner"])
def test_root_shape(check, kind):
    """The three BVHs have the roots the cases are about."""
    s, _ = check(kind)
    if kind == "leaves":
        assert (s["k_int"], s["leaf_tris"], s["nodes"]) == (0, 2, 1)
    elif kind == "mixed":
        assert 0 < s["k_int"] < 8 and s["leaf_tris"] > 0
    else:
        assert s["k_int"] == 8


@pytest.mark.parametrize("kind", ["leaves", "mixed", "inner"])
def test_rays_cover_the_cases(check, kind):
    """Every ray class is there in full; rays hit and miss the root, find triangles and occluders, and the
    shadow rays that end before the root box all miss it."""
    s, c = check(kind)
    assert s["rays"] == 2 * RAYS   # each ray as a closest-hit and as an any-hit query
    assert sorted(c) == sorted(CLASSES)
    for name in CLASSES:
        assert c[name]["rays"] == RAYS // len(CLASSES), name
    assert c["miss"]["root_miss"] == c["miss"]["rays"] and c["miss"]["found"] == 0
    assert c["shadow_before"]["found"] == 0
    for name in ("inside", "outside", "axis", "shadow_inside", "shadow_beyond"):
        assert 0 < c[name]["root_miss"] < c[name]["rays"], name
        assert c[name]["found"] > 0, name
    assert s["hits"] > 0 and s["occluded"] > 0
    # a query that reaches a root child starts one step later
    assert s["saved_steps"] == s["rays"] - s["root_miss"]


@pytest.mark.parametrize("kind", ["leaves", "mixed", "inner"])
def test_word_start_is_the_virtual_root_start(check, kind):
    s, _ = check(kind)
    for k in ("bad_hit", "bad_nodes", "bad_tris", "bad_order", "bad_steps"):
        assert s[k] == 0, f"{kind}: {k} = {s[k]} of {s['rays']} queries"


@pytest.mark.parametrize("kind", ["leaves", "mixed", "inner"])
def test_word_zero_is_todays_start(check, kind):
    s, _ = check(kind)
    assert s["bad_zero"] == 0, f"{kind}: {s['bad_zero']} of {s['rays']} queries"


@pytest.mark.parametrize("kind", ["leaves", "mixed", "inner"])
def test_against_the_serial_loop(check, kind):
    """trace8 finds the same hit bits, node visits and (closest hit) triangle tests."""
    s, _ = check(kind)
    assert s["bad_serial"] == 0, f"{kind}: {s['bad_serial']} of {s['rays']} queries"
