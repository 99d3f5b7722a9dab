"""Root words: wf_generate and wf_shade test the BVH root for every ray they append and hand wf_trace the
hit-slot mask, so a traced ray starts at the root's result.  The consumer applies exactly the
decision it would have made itself, so every frame here equals the CPU oracle bit for bit -- radiance, depth,
motion, closest and shadow ray counts -- with the finish threshold low enough that bulk rounds (the producers and
consumers of the words) run before the finish launch: one and two frames in flight, consecutive frames on one
slot (a stale word of the previous frame or round would show), the hit sort, the extra-sample pass (wf_extra
supplies no word: the "not supplied" start), a tile split with tile pixels outside the image, the counting
kernels (the root still counts as a node visit), and a glass case (front appends of refracting paths)."""
import json
import os
import sys

import numpy as np
import pytest

from helpers import parity_report

pytestmark = pytest.mark.gpu

W, H, SEED, TAIL = 128, 128, 7, 1024
CONFIGS = {"2spp4b": (2, 4), "1spp1b": (1, 1)}


def _renderer(rt, scene, w=W, h=H, **kw):
    return rt.Renderer(scene, w, h, pipeline="wavefront", tail_paths=TAIL, seed=SEED, **kw)


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


def _moved(rt, cam, dx):
    c = rt.Camera()
    c.position = type(cam.position)(cam.position.x + dx, cam.position.y, cam.position.z, 0.0)
    c.right, c.up, c.forward = cam.right, cam.up, cam.forward
    return c


@pytest.fixture(scope="module")
def c1(rt, assets):
    return rt.Scene.preset("c1", assets)


@pytest.fixture(scope="module")
def ref(rt, orc, c1):
    """Per configuration: the uniforms of two consecutive frames, the random offsets, and the oracle's two
    frames (every renderer of a configuration draws the same uniforms)."""
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
    """Two frames back to back.  One in flight: both on the same slot, each read and compared (the second
    reuses every queue and word array of the first).  Two in flight: the second overlaps the first."""
    spp, bounces = CONFIGS[cfg]
    R = _renderer(rt, c1, frames_in_flight=fif)
    R.samplesPerPixel, R.maxBounces = spp, bounces
    if fif == 1:
        for f in range(2):
            R.draw()
            got = _frame(R)
            _assert_oracle(got, ref[cfg][f], (cfg, f))
            st = R.stats()
            if bounces > 1:
                assert st.trace_launches >= 4, st.trace_launches   # two bulk rounds (extend + connect each) before the finish
    else:
        R.draw()
        R.draw()
        _assert_oracle(_frame(R), ref[cfg][1], cfg)
        assert R.stats().frames_in_flight == 2
    R.close()


def test_hit_sort(rt, c1, ref):
    """sort_bins=1024: wf_shade's sorted instance writes the words."""
    R = _renderer(rt, c1, sort_bins=1024)
    R.samplesPerPixel, R.maxBounces = CONFIGS["2spp4b"]
    for f in range(2):
        R.draw()
        _assert_oracle(_frame(R), ref["2spp4b"][f], f)
    R.close()


def test_counting_kernels(rt, c1, ref):
    """The counting instances: the same frame, and the root is still one node visit of every traced ray."""
    R = _renderer(rt, c1)
    R.samplesPerPixel, R.maxBounces = CONFIGS["2spp4b"]
    R.set_counting(True)
    R.draw()
    got = _frame(R)
    st = R.stats()
    R.close()
    _assert_oracle(got, ref["2spp4b"][0])
    assert st.node_visits > st.closest_rays + st.shadow_rays > 0
    assert st.trace_nodes >= st.trace_rays > 0   # every wf_trace ray visits at least the root


def test_extra_sample_pass(rt, orc, c1):
    """Motion-adaptive extra samples under a camera move: wf_extra's entries (word 0) pass through extend
    beside entries with words, in the arrays the base pass used."""
    spp, bounces = CONFIGS["2spp4b"]
    R = _renderer(rt, c1)
    R.samplesPerPixel, R.maxBounces = spp, bounces
    assert R.useMotionAdaptiveSampling
    cam0 = R.camera
    osc = orc.OracleScene(c1.desc())
    prev = motion = None
    for f in range(2):
        R.camera = _moved(rt, cam0, 0.4 * f)
        u = R.draw()
        got = _frame(R)
        o = osc.render(u, R.random, accum_in=prev, motion_in=motion)
        prev, motion = o["radiance"], o["motion"]
    R.close()
    assert o["paths"] > W * H * spp + TAIL   # extra samples ran, more of them than the finish threshold
    _assert_oracle(got, o)


def test_tile_split_outside_the_image(rt, orc, c1):
    """A 2-way split into 64-pixel tiles.  At 128 x 128 no tile pixel lies outside the image, so this case
    renders 120 x 100: rank 1's tiles (1 and 3) stick out to the right and at the bottom; their paths are
    never made, their queue entries and words never written.  Each rank's tiles equal the oracle's frame
    and the ranks' counts add up to its counts."""
    import torch
    w, h, T, n = 120, 100, 64, 2
    spp, bounces = CONFIGS["2spp4b"]
    tx = (w + T - 1) // T
    canvas = total = o = None
    for rank in (1, 0):
        R = _renderer(rt, c1, w, h)
        R.samplesPerPixel, R.maxBounces = spp, bounces
        u = R.draw(tiles=(T, rank, n))
        if o is None:
            o = orc.OracleScene(c1.desc()).render(u, R.random)
            canvas = np.zeros_like(o["radiance"])
            total = np.zeros(3, np.int64)
        cnt = R.tile_count(T, rank, n)
        buf = torch.empty((cnt, T, T, 4), dtype=torch.float32, device="cuda")
        R.pack_tiles(T, rank, n, buf.data_ptr())
        R.wait()
        torch.cuda.synchronize()
        packed = buf.cpu().numpy()
        st = R.stats()
        total += (st.closest_rays, st.shadow_rays, st.paths)
        R.close()
        for k in range(cnt):
            tid = rank + k * n
            x0, y0 = (tid % tx) * T, (tid // tx) * T
            ww, hh = min(T, w - x0), min(T, h - y0)
            assert ww > 0 and hh > 0
            canvas[y0:y0 + hh, x0:x0 + ww] = packed[k, :hh, :ww, :canvas.shape[-1]]
            assert np.array_equal(packed[k, :hh, :ww, :3], o["radiance"][y0:y0 + hh, x0:x0 + ww, :3]), (rank, k)
    assert np.array_equal(canvas[..., :3], o["radiance"][..., :3])
    assert tuple(total) == (o["closest_rays"], o["shadow_rays"], o["paths"])


def test_glass_front_appends(rt, assets):
    """The committed glass fixture (C3g, 8 bounces) with a finish threshold of 64 paths: refracting paths'
    continuation rays are appended at the queue fronts, their words beside them."""
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
    assert st.trace_launches >= 4
