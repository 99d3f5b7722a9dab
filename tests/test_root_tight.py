"""The exact root boxes (csrc/rt_device.h RootBoxes, root_boxes_fill, root_word_tight), evaluated on the host:
tools/root_tight_check.cpp is compiled with plain g++ together with the BVH builder and steps seeded rays against
four small BVHs -- roots that are all leaves, internal children beside leaf triangles, eight internal children,
and a flat floor quad as a leaf of a root more than 100 times as high as the quad's box is thick (the case the
8-bit root grid stores as a thick slab).  Every query runs from the virtual root group and from the tight word,
closest-hit and any-hit.  The hit records must agree bit for bit, a mask of 0 (the ray its producer retires) must
never come with a hit, an empty slot never gets a bit -- and the tight masks must really differ from the
quantised ones in every ray class, so the comparison exercises the difference."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PER_CLASS = 600
KINDS = ["leaves", "mixed", "inner", "floor"]
CLASSES = ["away", "toward", "parallel", "vertex", "edge", "corner", "axis", "shadow_before", "shadow_beyond",
           "inside", "outside"]


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("root_tight")), "root_tight_check")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off",
                    "-D__HIP_PLATFORM_AMD__", "-I", ROOT, "-I", os.path.join(rocm, "include"),
                    os.path.join(ROOT, "tools", "root_tight_check.cpp"),
                    os.path.join(ROOT, "metal4-raytracing_amd", "csrc", "rt_bvh.cpp"), "-o", exe], check=True)
    cache = {}

    def run(kind):
        """(summary fields, per-class fields) of the tool's answer for a root of `kind`."""
        if kind not in cache:
            r = subprocess.run([exe, kind, str(PER_CLASS)], capture_output=True, text=True, timeout=120, check=True)
            lines = r.stdout.split("\n")[:-1]
            head = lines[0].split()
            assert head[0] == kind
            summary = {k: float(v) for k, v in zip(head[1::2], head[2::2])}
            classes = {}
            for line in lines[1:]:
                w = line.split()
                assert w[0] == "class"
                classes[w[1]] = {k: int(v) for k, v in zip(w[2::2], w[3::2])}
            cache[kind] = (summary, classes)
        return cache[kind]
    return run


@pytest.mark.parametrize("kind", KINDS)
def test_root_shape(check, kind):
    """The BVHs have the roots the cases are about; the floor case reproduces the thick slab."""
    s, _ = check(kind)
    if kind == "leaves":
        assert (s["k_int"], s["leaf_tris"], s["nodes"]) == (0, 4, 1)
    elif kind == "mixed":
        assert 0 < s["k_int"] < 8 and s["leaf_tris"] > 0
    elif kind == "inner":
        assert s["k_int"] == 8
    else:
        assert s["flat_slot"] >= 0
        # the root is at least 100 times as high as the quad's exact box is thick (the quad itself: 0) ...
        assert s["root_extent"] >= 100.0 * s["flat_thick"] > 0.0
        # ... while its quantised box is far thicker than a continuation ray's 1e-3 offset
        assert s["quant_thick"] >= 10.0 * 1e-3


@pytest.mark.parametrize("kind", KINDS)
def test_rays_cover_the_cases(check, kind):
    """Every ray class is there in full, as closest-hit and any-hit queries; rays find triangles and occluders,
    and some are retired."""
    s, c = check(kind)
    assert sorted(c) == sorted(CLASSES)
    for name in CLASSES:
        assert c[name]["rays"] == 2 * PER_CLASS, name
    assert s["queries"] == 2 * PER_CLASS * len(CLASSES)
    assert s["hits"] > 0 and s["occluded"] > 0 and s["retired"] > 0
    assert c["toward"]["found"] == c["toward"]["rays"] and c["toward"]["zero"] == 0
    assert c["shadow_beyond"]["found"] == c["shadow_beyond"]["rays"]
    assert c["parallel"]["found"] == 0


@pytest.mark.parametrize("kind", KINDS)
def test_tight_start_is_the_virtual_root_start(check, kind):
    s, _ = check(kind)
    for k in ("bad_hit", "bad_zero", "bad_empty"):
        assert s[k] == 0, f"{kind}: {k} = {s[k]} of {s['queries']} queries"


@pytest.mark.parametrize("kind", KINDS)
def test_tight_masks_differ(check, kind):
    """In every class but "toward" some tight masks are strict subsets of the quantised ones."""
    _, c = check(kind)
    for name in CLASSES:
        if name != "toward":
            assert c[name]["tighter"] > 0, (kind, name)
