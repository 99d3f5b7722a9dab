"""Exact root boxes: wf_generate and wf_shade test every ray they make against the fp32 bounds of the BVH root's
children (root_word_tight) and do not enqueue a closest-hit ray whose mask is 0 -- a proven miss (DESIGN.md
§3.1).  A retired ray ends its path exactly as the miss record would have, so every frame here equals the CPU
oracle bit for bit -- radiance, depth, motion, closest and shadow ray counts -- with the finish threshold low
enough that bulk rounds (the producers) run before the finish launch: consecutive frames on one slot, two frames
in flight, the hit sort, a camera turned so that primary rays leave the scene (wf_generate retires them), a refit
after an instance move (the boxes follow the geometry), the counting kernels (a retired ray still counts its root
visit), and the glass fixture."""
import json
import math
import os
import sys

import numpy as np
import pytest

from helpers import parity_report

pytestmark = pytest.mark.gpu

W, H, SEED, TAIL = 128, 128, 7, 1024
CONFIGS = {"2spp4b": (2, 4), "1spp1b": (1, 1)}


def _renderer(rt, scene, **kw):
    return rt.Renderer(scene, W, H, pipeline="wavefront", tail_paths=TAIL, seed=SEED, **kw)


def _frame(R):
    R.wait()
    depth, motion, _ = R.aux()
    st = R.stats()
    return R.radiance(), depth, motion, (st.closest_rays, st.shadow_rays, st.paths)


def _assert_oracle(got, o, what=""):
    g, depth, motion, counts = got
    assert np.array_equal(g[..., :3], o["radiance"][..., :3]), what
    assert np.array_equal(depth, o["depth"]) and np.array_equal(motion, o["motion"]), what
    assert counts == (o["closest_rays"], o["shadow_rays"], o["paths"]), what


def _assert_counters(st):
    """A retired ray counts where the miss wf_trace would have resolved counts."""
    assert st.root_retired_rays <= st.trace_closest_rays <= st.closest_rays
    assert st.trace_closest_rays <= st.trace_rays <= st.closest_rays + st.shadow_rays


def _turned(rt, cam, degrees):
    """The camera turned about its up vector."""
    V = type(cam.position)
    c, s = math.cos(math.radians(degrees)), math.sin(math.radians(degrees))
    f, r = cam.forward, cam.right
    t = rt.Camera()
    t.position, t.up = cam.position, cam.up
    t.forward = V(c * f.x + s * r.x, c * f.y + s * r.y, c * f.z + s * r.z, 0.0)
    t.right = V(c * r.x - s * f.x, c * r.y - s * f.y, c * r.z - s * f.z, 0.0)
    return t


@pytest.fixture(scope="module")
def c1(rt, assets):
    return rt.Scene.preset("c1", assets)


@pytest.fixture(scope="module")
def ref(rt, orc, c1):
    """Per configuration: the oracle's two consecutive frames (every renderer of a configuration draws the
    same uniforms)."""
    osc = orc.OracleScene(c1.desc())
    out = {}
    for name, (spp, bounces) in CONFIGS.items():
        R = _renderer(rt, c1)
        R.samplesPerPixel, R.maxBounces = spp, bounces
        us = [R.draw() for _ in range(2)]
        R.wait()
        rnd = R.random
        R.close()
        prev = motion = None
        frames = []
        for u in us:
            o = osc.render(u, rnd, accum_in=prev, motion_in=motion)
            prev, motion = o["radiance"], o["motion"]
            frames.append(o)
        out[name] = frames
    return out


@pytest.mark.parametrize("fif", [1, 2])
@pytest.mark.parametrize("cfg", sorted(CONFIGS))
def test_consecutive_frames(rt, c1, ref, cfg, fif):
    """Two frames back to back.  One in flight: both on the same slot, each read and compared.  Two in flight:
    the second overlaps the first."""
    spp, bounces = CONFIGS[cfg]
    R = _renderer(rt, c1, frames_in_flight=fif)
    R.samplesPerPixel, R.maxBounces = spp, bounces
    if fif == 1:
        for f in range(2):
            R.draw()
            _assert_oracle(_frame(R), ref[cfg][f], (cfg, f))
            _assert_counters(R.stats())
    else:
        R.draw()
        R.draw()
        _assert_oracle(_frame(R), ref[cfg][1], cfg)
        assert R.stats().frames_in_flight == 2
        _assert_counters(R.stats())
    R.close()


def test_hit_sort(rt, c1, ref):
    """sort_bins=1024: wf_shade's sorted instance makes the words and retires."""
    R = _renderer(rt, c1, sort_bins=1024)
    R.samplesPerPixel, R.maxBounces = CONFIGS["2spp4b"]
    for f in range(2):
        R.draw()
        _assert_oracle(_frame(R), ref["2spp4b"][f], f)
        _assert_counters(R.stats())
    R.close()


@pytest.mark.parametrize("cfg", sorted(CONFIGS))
def test_turned_camera_retires_primary_rays(rt, orc, c1, cfg):
    """The camera turned by 60 degrees: part of the primary rays leave the scene, wf_generate retires them, and
    the frame and its ray counts are the oracle's."""
    spp, bounces = CONFIGS[cfg]
    R = _renderer(rt, c1)
    R.samplesPerPixel, R.maxBounces = spp, bounces
    R.camera = _turned(rt, R.camera, 60.0)
    u = R.draw()
    got = _frame(R)
    st = R.stats()
    rnd = R.random
    R.close()
    o = orc.OracleScene(c1.desc()).render(u, rnd)
    print(cfg, "root_retired_rays", st.root_retired_rays, "closest", st.closest_rays, "trace_closest", st.trace_closest_rays)
    _assert_oracle(got, o, cfg)
    assert np.any(o["depth"] == np.float32(1.0e8)), "no primary ray leaves the scene"
    assert st.root_retired_rays > 0
    assert st.total_root_retired_rays == st.root_retired_rays
    _assert_counters(st)


def test_counting_kernels(rt, orc, c1):
    """The counting instances with the turned camera: the same frame, closest + shadow rays equal the oracle's,
    and every traced ray -- a retired one too -- has visited at least the root."""
    R = _renderer(rt, c1)
    R.samplesPerPixel, R.maxBounces = CONFIGS["2spp4b"]
    R.camera = _turned(rt, R.camera, 60.0)
    R.set_counting(True)
    u = R.draw()
    got = _frame(R)
    st = R.stats()
    rnd = R.random
    R.close()
    o = orc.OracleScene(c1.desc()).render(u, rnd)
    _assert_oracle(got, o)
    assert st.closest_rays + st.shadow_rays == o["closest_rays"] + o["shadow_rays"]
    assert st.root_retired_rays > 0
    assert st.trace_nodes >= st.trace_rays > 0
    assert st.node_visits >= st.closest_rays + st.shadow_rays
    _assert_counters(st)


def test_refit_after_instance_move(rt, orc, c1):
    """set_instance_transforms + refit between two frames: the root boxes are refilled after the refit, so the
    moved mesh is found where it now is."""
    from test_gpu_dynamic import _desc_with
    desc = c1.desc()
    R = _renderer(rt, c1)
    R.samplesPerPixel, R.maxBounces = CONFIGS["2spp4b"]
    u0 = R.draw()
    R.wait()
    o0 = orc.OracleScene(desc).render(u0, R.random)
    _assert_oracle(_frame(R), o0, 0)
    mats = np.stack([np.frombuffer(bytes(desc.meshes[k].transform), np.float32).reshape(4, 3).copy()
                     for k in range(desc.mesh_count)])
    old0 = mats[0].copy()
    mats[0, 3, 0] += 0.6
    mats[0, 3, 1] += 0.3
    R.set_instance_transforms(mats)
    R.refit()
    u1 = R.draw()
    got = _frame(R)
    st = R.stats()
    rnd = R.random
    R.close()
    osc1 = orc.OracleScene(_desc_with(rt, desc, 0, transform=mats[0]))
    osc1.set_previous(0, prev_transform=old0)
    o1 = osc1.render(u1, rnd, accum_in=o0["radiance"], motion_in=o0["motion"])
    _assert_oracle(got, o1, 1)
    assert not np.array_equal(o1["depth"], o0["depth"])   # the move shows
    _assert_counters(st)


def test_glass_fixture(rt, assets):
    """The committed glass fixture (C3g, 8 bounces) with a finish threshold of 64 paths."""
    from conftest import ROOT
    gdir = os.path.join(ROOT, "tests", "golden")
    name = "c3g_small_b8"
    meta = json.load(open(os.path.join(gdir, "cases.json")))[name]
    g = np.load(os.path.join(gdir, name + ".npz"))
    sys.path.insert(0, gdir)
    import make_golden
    scene = make_golden.make_scene(rt, meta["preset"], assets)
    R = rt.Renderer(scene, meta["width"], meta["height"], pipeline="wavefront", tail_paths=64, seed=meta["seed"])
    for k, v in meta["knobs"].items():
        setattr(R, k, v)
    for _ in range(meta["frames"]):
        R.draw()
    R.wait()
    img = R.radiance()[..., :3]
    depth, motion, _ = R.aux()
    st = R.stats()
    R.close()
    rep = parity_report(img, g["radiance"])
    assert rep["n_bad"] == 0, rep
    assert np.array_equal(img, g["radiance"])
    assert np.array_equal(depth, g["depth"]) and np.array_equal(motion, g["motion"])
    assert [st.closest_rays, st.shadow_rays] == g["counts"].tolist()[:2]
    print("c3g_small_b8 root_retired_rays", st.root_retired_rays, "closest", st.closest_rays)
    assert st.root_retired_rays > 0   # continuation rays leave the open scene
    _assert_counters(st)
