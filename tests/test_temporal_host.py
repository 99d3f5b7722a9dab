"""The temporal host hooks on CPU (include/rt_api.h: rt_debug_primary_outputs_host,
rt_debug_extra_paths_host, rt_debug_resolve_samples_host; per-record code in csrc/rt_paths.h around
primary_outputs / extra_samples / resolve_pixel of csrc/rt_shade.h, the frame kernels' own
functions compiled for the host): the new struct against the header compiled with gcc, and frames
after the first assembled from the hooks against the oracle: a moved instance with motion-adaptive
extra samples and the EMA, glass paths whose sample 0 has several bounce-0 hits, and the
resolve's arithmetic and error returns.  Every comparison is bitwise."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import shade_ref as sh
import surface_ref as sr
from conftest import ROOT

F = np.float32
ALIVE = 1
NEW_SYMBOLS = ["rt_debug_primary_outputs_host", "rt_debug_extra_paths_host", "rt_debug_resolve_samples_host"]


def same(a, b):
    return np.array_equal(sr.bits(a), sr.bits(b))


class DescScene:
    """A scene descriptor built in the test, for the hooks (which only call desc())."""

    def __init__(self, d):
        self._d = d

    def desc(self):
        return self._d


def desc_with_transform(rt, desc, mesh, transform):
    """A copy of desc whose mesh `mesh` has another transform (as tests/test_gpu_dynamic.py moves it)."""
    A = rt._abi
    arr = (A.MeshDesc * desc.mesh_count)()
    for m in range(desc.mesh_count):
        C.pointer(arr[m])[0] = desc.meshes[m]
    C.memmove(C.byref(arr[mesh].transform), np.ascontiguousarray(transform, np.float32).ctypes.data, 48)
    d = A.SceneDesc()
    d.mesh_count, d.light_count, d.meshes, d.lights = desc.mesh_count, desc.light_count, arr, desc.lights
    d.texture_count, d.textures = desc.texture_count, desc.textures
    d._keep = (arr,)
    return d


def transforms(desc):
    return np.stack([np.frombuffer(bytes(desc.meshes[k].transform), np.float32).reshape(4, 3).copy()
                     for k in range(desc.mesh_count)])


def frame_uniforms(rt, scene, W, H, frame, spp, bounces):
    u = rt.uniforms_default(W, H, scene.desc().light_count)
    u.camera = rt.camera_default(W, H)
    u.previousCamera = u.camera
    u.frameIndex, u.samplesPerPixel, u.maxBounces = frame, spp, bounces
    return u


def rounds(rt, B, rays, paths, samples, guard, primary=None):
    """The query loop over host arrays, compacting with numpy: trace -> resolve -> primary ->
    shade -> shadow rays -> connect -> retire by tag -> the live records go on.  Returns (closest
    rays, shadow rays, rounds)."""
    closest = shadows = n_rounds = 0
    while len(paths):
        assert n_rounds < guard
        hits = B.trace(rays)
        S = B.resolve(rays, hits)
        if primary is not None:
            primary(hits, paths)
        out = B.shade(rays, S, paths)
        p = out.paths
        shm = p.shadow
        if shm.any():
            occluded = B.trace_any(out.shadow_rays[shm])
            lit = shm.copy()
            lit[shm] = occluded == 0
            p.radiance[:] = np.where(lit[:, None], p.radiance + out.contrib[:, 0:3], p.radiance)
        dead = ~p.alive
        samples[p.tag[dead], 0:3] = p.radiance[dead]
        samples[p.tag[dead], 3] = 1.0
        closest += len(paths)
        shadows += int(shm.sum())
        alive = p.alive
        rays = np.ascontiguousarray(out.next_rays[alive])
        pb = np.ascontiguousarray(p.buffer[alive])
        paths = rt.Paths(pb, pb.view(np.int32))
        n_rounds += 1
    return closest, shadows, n_rounds


def host_frame(rt, scene, u, rnd, history=None, prev_transforms=None):
    """A frame from the host hooks alone, in the renderer's order (base pass, extra samples, resolve).  history: dict(radiance,
    motion) of the previous frame.  Returns dict(radiance (H, W, 4), depth, motion, extra,
    closest_rays, shadow_rays, paths)."""
    W, H, spp, mb = u.width, u.height, u.samplesPerPixel, u.maxBounces
    pixels = W * H
    me = max(u.motionSamplingMaxExtraSamples, 0) if u.enableMotionAdaptiveSampling else 0
    stride = spp + me
    B = sh.HostBackend(rt, scene, u.shadingMode, mb, u.lightCount)
    depth, motion = np.full(pixels, 1.0e8, F), np.zeros((pixels, 2), F)     # what a pixel holds before its sample 0 runs
    samples = np.full((pixels * stride, 4), np.nan, F)

    def primary(hits, paths):
        rt.debug_primary_outputs_host(scene, u, hits, paths, depth, motion, tag_stride=stride, tag_offset=0,
                                      prev_transforms=prev_transforms)

    base = [rt.debug_camera_paths_host(u, rnd, s, tag_stride=stride, tag_offset=s) for s in range(spp)]
    rays = np.concatenate([r for r, _ in base])
    pb = np.concatenate([p.buffer for _, p in base])
    guard = sh.guard_steps(mb)
    nc, ns, _ = rounds(rt, B, rays, rt.Paths(pb, pb.view(np.int32)), samples, guard, primary)
    prev_motion = history["motion"] if history is not None else None
    erays, epaths, extra = rt.debug_extra_paths_host(u, rnd, motion, prev_motion, tag_stride=stride, tag_offset=spp)
    live = (epaths.flags & ALIVE) != 0                                       # rt_compact_paths(RT_PATH_ALIVE)
    assert int(live.sum()) == int(extra.sum())
    eb = np.ascontiguousarray(epaths.buffer[live])
    ec, es, _ = rounds(rt, B, np.ascontiguousarray(erays[live]), rt.Paths(eb, eb.view(np.int32)), samples, guard)
    rgba = rt.debug_resolve_samples_host(u, samples, stride, extra=extra, motion=motion, motion_prev=prev_motion,
                                         history=history["radiance"] if history is not None else None)
    return dict(radiance=rgba.reshape(H, W, 4), depth=depth.reshape(H, W), motion=motion.reshape(H, W, 2), extra=extra,
                closest_rays=nc + ec, shadow_rays=ns + es, paths=pixels * spp + int(extra.sum()))


def assert_frame_equals_oracle(got, o):
    assert same(got["radiance"], o["radiance"])
    assert same(got["depth"], o["depth"])
    assert same(got["motion"], o["motion"])
    assert (got["closest_rays"], got["shadow_rays"], got["paths"]) == (o["closest_rays"], o["shadow_rays"], o["paths"])


# ---- 1. layout and symbols -------------------------------------------------------------------
def test_target_opts_layout_matches_c(rt, tmp_path):
    A = rt._abi
    lines = ["P(rt_target_opts);"] + [f"O(rt_target_opts, {f});" for f, _ in A.TargetOpts._fields_]
    prog = tmp_path / "tlayout.c"
    prog.write_text(r'''
#include <stdio.h>
#include <stddef.h>
#include "rt_api.h"
#define P(T) printf(#T " %zu\n", sizeof(T))
#define O(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))
int main(void) {
  ''' + "\n  ".join(lines) + r'''
  return 0;
}''')
    exe = tmp_path / "tlayout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    out = dict(line.rsplit(" ", 1) for line in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(out["rt_target_opts"]) == C.sizeof(A.TargetOpts) == 32
    for f, _ in A.TargetOpts._fields_:
        assert int(out[f"rt_target_opts.{f}"]) == getattr(A.TargetOpts, f).offset, f
    assert (A.TargetOpts.tag_stride.offset, A.TargetOpts.tag_offset.offset, A.TargetOpts.pixels.offset) == (0, 4, 8)


def test_temporal_hooks_resolve(rt):
    lib, A = rt.lib(), rt._abi
    for name in NEW_SYMBOLS:
        assert name in A.EXPORTED_SYMBOLS, name
        assert getattr(lib, name).argtypes is not None, name
    for name in ("debug_primary_outputs_host", "debug_extra_paths_host", "debug_resolve_samples_host"):
        assert callable(getattr(rt, name)), name


# ---- 2. c2: a moved instance, extra samples, the EMA -----------------------------------------------------
C2 = dict(W=96, H=64, seed=9, spp=1, bounces=2, shift=0.3)
_C2 = {}


def c2_case(rt, orc, assets):
    """Frames 0 (still) and 1 (mesh 0 translated by +0.3 in x) of c2 at 96 x 64 by the oracle, prepared
    as test_instance_motion_and_extra_samples prepares it.  Computed once, never modified."""
    if not _C2:
        W, H = C2["W"], C2["H"]
        sc = rt.Scene.preset("c2", assets)
        desc = sc.desc()
        rnd = rt.random_offsets(C2["seed"], W, H)
        u0 = frame_uniforms(rt, sc, W, H, 0, C2["spp"], C2["bounces"])
        u1 = frame_uniforms(rt, sc, W, H, 1, C2["spp"], C2["bounces"])
        assert u1.enableMotionAdaptiveSampling and u1.motionSamplingMaxExtraSamples == 2   # default knobs
        o0 = orc.OracleScene(desc).render(u0, rnd)
        mats = transforms(desc)
        old0 = mats[0].copy()
        mats[0, 3, 0] += C2["shift"]
        # a scene of its own under the moved descriptor: Scene.desc() rebuilds the arrays earlier
        # descriptors of the same scene point to, and the hooks call it on `sc`
        sc1 = rt.Scene.preset("c2", assets)
        d1 = desc_with_transform(rt, sc1.desc(), 0, mats[0])
        osc1 = orc.OracleScene(d1)
        osc1.set_previous(0, prev_transform=old0)
        o1 = osc1.render(u1, rnd, accum_in=o0["radiance"], motion_in=o0["motion"])
        prev = mats.copy()
        prev[0] = old0
        _C2.update(scene=sc, moved=DescScene(d1), rnd=rnd, u0=u0, u1=u1, o0=o0, o1=o1, prev=prev, keep=(old0, osc1, sc1))
    return _C2


def test_c2_extra_histogram_equals_oracle_paths(rt, orc, assets):
    c = c2_case(rt, orc, assets)
    pixels = C2["W"] * C2["H"]
    _, paths, extra = rt.debug_extra_paths_host(c["u1"], c["rnd"], c["o1"]["motion"], c["o0"]["motion"], tag_stride=3,
                                                tag_offset=1)
    hist = np.bincount(extra, minlength=3)
    assert len(hist) == 3 and np.all(hist > 0), hist        # every exercised value of e occurs
    assert hist.tolist() == [5834, 11, 299]
    assert int(extra.sum()) == c["o1"]["paths"] - pixels == 609
    # the records: maxExtra per pixel, the first extra[i] live with the tags of samples spp + j
    assert len(paths) == pixels * 2
    live = (paths.flags.reshape(pixels, 2) & ALIVE) != 0
    assert np.array_equal(live, np.arange(2)[None, :] < extra[:, None])
    want = (np.arange(pixels)[:, None] * 3 + 1 + np.arange(2)[None, :]).astype(np.int32)
    assert np.array_equal(paths.tag.reshape(pixels, 2)[live], want[live])
    dead = paths.buffer.reshape(pixels, 2, 12)[~live]
    assert not dead.view(np.uint32).any()


def test_c2_frames_from_hooks_equal_oracle(rt, orc, assets):
    c = c2_case(rt, orc, assets)
    f0 = host_frame(rt, c["scene"], c["u0"], c["rnd"])
    assert_frame_equals_oracle(f0, c["o0"])
    assert not f0["extra"].any()
    hist = dict(radiance=c["o0"]["radiance"], motion=c["o0"]["motion"])
    f1 = host_frame(rt, c["moved"], c["u1"], c["rnd"], history=hist, prev_transforms=c["prev"])
    assert_frame_equals_oracle(f1, c["o1"])
    assert np.abs(f1["motion"]).max() > 0 and f1["paths"] == 6753
    # without the old transform the motion is not the oracle's: prev_transforms is what gives it
    still = host_frame(rt, c["moved"], c["u1"], c["rnd"], history=hist)
    assert not still["motion"].any() and same(still["depth"], c["o1"]["depth"])


# ---- 3. glass: the last bounce-0 hit of sample 0 wins ------------------------------------------------------
def test_glass_last_bounce0_hit_wins(rt, orc, assets):
    W, H = 64, 36
    sc = rt.Scene.preset("c3g", assets)
    rnd = rt.random_offsets(11, W, H)
    u = frame_uniforms(rt, sc, W, H, 0, 1, 8)
    osc = orc.OracleScene(sc.desc())
    o = osc.render(u, rnd)
    # Only the bounce-0 part of the paths matters here, so the loop keeps the records that are still
    # at bounce 0 and traces no shadow ray (radiance is not compared).  The scene has 881 K
    # triangles and debug_trace_host builds its tree on every call (seconds), so the closest hits
    # come from the oracle's intersector ray by ray: the same t, u, v, or the depths would differ.
    lights = sh.scene_lights(sc)
    rays, paths = rt.debug_camera_paths_host(u, rnd, 0)
    depth, motion = np.full(W * H, 1.0e8, F), np.zeros((W * H, 2), F)
    first = None
    hits_per_pixel = np.zeros(W * H, np.int32)
    for rnd_no in range(u.maxBounces + 1):
        if not len(paths):
            break
        assert rnd_no < u.maxBounces
        hits = np.broadcast_to(sh.MISS_HIT.view(F), (len(paths), 8)).copy()
        for k in range(len(paths)):
            h = osc.intersect(rays[k, 0:3], rays[k, 4:7])
            if h is not None:
                hits[k, 0:3] = (h[0], h[2], h[3])
                hits.view(np.uint32)[k, 3] = h[1]
        hit = hits.view(np.uint32)[:, 3] != sr.MISS
        np.add.at(hits_per_pixel, paths.tag[hit], 1)
        rt.debug_primary_outputs_host(sc, u, hits, paths, depth, motion)
        if first is None:
            first = depth.copy()
        S = rt.debug_resolve_host(sc, rays, hits)
        out = rt.debug_shade_host(lights, rays, S, paths, max_bounces=u.maxBounces)
        go = out.paths.alive & (out.paths.bounce == 0)
        rays = np.ascontiguousarray(out.next_rays[go])
        pb = np.ascontiguousarray(out.paths.buffer[go])
        paths = rt.Paths(pb, pb.view(np.int32))
    assert same(depth.reshape(H, W), o["depth"]) and same(motion.reshape(H, W, 2), o["motion"])
    several = hits_per_pixel >= 2
    assert several.sum() == 52 and hits_per_pixel.max() == 7
    # applying only round 1's hits is not enough, and it is wrong exactly where a later hit exists
    differ = sr.bits(first.reshape(H, W)) != sr.bits(o["depth"])
    assert differ.any() and not differ.reshape(-1)[~several].any()


# ---- 4. resolve_samples: arithmetic and errors -------------------------------------------------------------
def test_resolve_samples_frame0_equals_average(rt):
    rng = np.random.default_rng(4)
    pixels = 257
    for spp in (1, 3, 64):
        u = rt.uniforms_default(pixels, 1)
        u.frameIndex, u.samplesPerPixel, u.enableMotionAdaptiveSampling = 0, spp, 0
        s = rng.uniform(0, 4, (pixels * spp, 4)).astype(F)
        total = s.reshape(pixels, spp, 4)[:, 0, 0:3].copy()
        for k in range(1, spp):
            total = total + s.reshape(pixels, spp, 4)[:, k, 0:3]
        want = np.concatenate([total / F(spp), np.ones((pixels, 1), F)], axis=1)    # average_pixel's arithmetic
        assert same(rt.debug_resolve_samples_host(u, s, spp), want)
        # a wider stride and an all-zero extra read the same samples
        wide = np.full((pixels, spp + 2, 4), np.nan, F)
        wide[:, :spp] = s.reshape(pixels, spp, 4)
        assert same(rt.debug_resolve_samples_host(u, wide, spp + 2, extra=np.zeros(pixels, np.uint32)), want)


def test_resolve_samples_extra_and_ema(rt):
    rng = np.random.default_rng(5)
    pixels, spp, me = 130, 2, 3
    u = rt.uniforms_default(pixels, 1)
    u.frameIndex, u.samplesPerPixel = 3, spp
    u.enableMotionAdaptiveSampling, u.motionSamplingMaxExtraSamples = 1, me
    assert u.enableMotionAdaptiveAccumulation
    s = rng.uniform(0, 4, (pixels, spp + me, 4)).astype(F)
    extra = rng.integers(0, me + 1, pixels).astype(np.uint32)
    motion = rng.uniform(-8, 8, (pixels, 2)).astype(F)
    motion[::3] = 0
    prev = rng.uniform(-8, 8, (pixels, 2)).astype(F)
    prev[::2] = 0
    history = rng.uniform(0, 4, (pixels, 4)).astype(F)
    got = rt.debug_resolve_samples_host(u, s, spp + me, extra=extra, motion=motion, motion_prev=prev, history=history)
    # resolve_pixel (csrc/rt_shade.h) restated in numpy float32, one operation per line
    count = spp + extra
    total = s[:, 0, 0:3].copy()
    for k in range(1, spp + me):
        total = np.where((k < count)[:, None], total + s[:, k, 0:3], total)
    total = total / count.astype(F)[:, None]
    hw = np.minimum(np.maximum(F(u.accumulationWeight), F(0)), F(0.95))
    mag = np.maximum(np.sqrt(motion[:, 0] * motion[:, 0] + motion[:, 1] * motion[:, 1]),
                     np.sqrt(prev[:, 0] * prev[:, 0] + prev[:, 1] * prev[:, 1]))
    low = np.maximum(F(u.motionAccumulationLowThresholdPixels), F(0))
    high = np.maximum(F(u.motionAccumulationHighThresholdPixels), low + F(1e-3))
    t = np.minimum(np.maximum((mag - low) / (high - low), F(0)), F(1))
    mw = np.minimum(np.minimum(np.maximum(F(u.motionAccumulationMinWeight), F(0)), F(0.95)), hw)
    w = hw + (mw - hw) * t
    want = total + (history[:, 0:3] - total) * w[:, None]
    assert same(got[:, 0:3], want) and np.all(got[:, 3] == 1)
    assert len(np.unique(w)) > 3                                # still, moving and in between
    # an extra above what the stride holds counts as the stride's
    big = extra.copy()
    big[:] = 1000
    full = np.full(pixels, me, np.uint32)
    assert same(rt.debug_resolve_samples_host(u, s, spp + me, extra=big, motion=motion, motion_prev=prev, history=history),
                rt.debug_resolve_samples_host(u, s, spp + me, extra=full, motion=motion, motion_prev=prev, history=history))


def test_resolve_samples_errors(rt):
    L, A = rt.lib(), rt._abi
    E = A.RT_ERR_INVALID_ARG
    pixels, spp = 8, 2
    u = rt.uniforms_default(pixels, 1)
    u.frameIndex, u.samplesPerPixel = 0, spp
    u.enableMotionAdaptiveSampling, u.motionSamplingMaxExtraSamples = 1, 2
    s, out, hist = np.zeros((pixels * 4 + 1, 4), F), np.zeros((pixels + 1, 4), F), np.zeros((pixels, 4), F)
    mv, ex = np.zeros((pixels + 1, 2), F), np.zeros(pixels + 1, np.uint32)

    def call(un=u, smp=s.ctypes.data, stride=4, extra=None, motion=None, prev=None, history=None, n=pixels, rgba=out.ctypes.data):
        return L.rt_debug_resolve_samples_host(C.byref(un) if un is not None else None, smp, stride, extra, motion, prev,
                                               history, n, rgba)

    assert call() == A.RT_OK
    assert call(stride=3) == E                                   # spp + maxExtra > sample_stride
    off = rt.uniforms_default(pixels, 1)
    off.samplesPerPixel, off.enableMotionAdaptiveSampling = spp, 0
    assert call(un=off, stride=2) == A.RT_OK and call(un=off, stride=1) == E
    later = rt.uniforms_default(pixels, 1)
    later.frameIndex, later.samplesPerPixel, later.enableMotionAdaptiveSampling = 1, spp, 0
    assert call(un=later) == E                                   # history == NULL at frame > 0
    assert call(un=later, history=hist.ctypes.data) == A.RT_OK
    assert call(un=later, history=out.ctypes.data) == E          # rgba aliases history
    for bad in (0, 65):
        b = rt.uniforms_default(pixels, 1)
        b.samplesPerPixel, b.enableMotionAdaptiveSampling = bad, 0
        assert call(un=b, stride=80) == E
    assert call(un=None) == E and call(smp=None) == E and call(rgba=None) == E
    assert call(smp=None, rgba=None, n=0) == A.RT_OK
    assert call(smp=s.ctypes.data + 4) == E and call(rgba=out.ctypes.data + 8) == E
    assert call(motion=mv.ctypes.data + 4) == E and call(extra=ex.ctypes.data + 2) == E
    assert call(smp=s.ctypes.data + 16, rgba=out.ctypes.data + 16, motion=mv.ctypes.data + 8, extra=ex.ctypes.data + 4) == A.RT_OK
    with pytest.raises(rt.RTError):
        rt.debug_resolve_samples_host(later, s[:pixels * 4], 4)


def test_primary_and_extra_hooks_reject_bad_arguments(rt, assets):
    L, A = rt.lib(), rt._abi
    E = A.RT_ERR_INVALID_ARG
    W, H = 7, 5
    sc = rt.Scene.preset("c1", assets)
    d = sc.desc()
    u = frame_uniforms(rt, sc, W, H, 0, 1, 2)
    hits, paths = np.zeros((4, 8), F), np.zeros((4, 12), F)
    depth, motion = np.zeros(W * H + 1, F), np.zeros((W * H + 1, 2), F)

    def primary(stride=1, offset=0, h=hits.ctypes.data, p=paths.ctypes.data, dp=depth.ctypes.data, mv=motion.ctypes.data, n=4,
                un=u, scene=d):
        o = A.TargetOpts()
        o.tag_stride, o.tag_offset, o.pixels = stride, offset, W * H
        return L.rt_debug_primary_outputs_host(C.byref(scene) if scene is not None else None, None,
                                               C.byref(un) if un is not None else None, C.byref(o), h, p, n, dp, mv)

    assert primary() == A.RT_OK
    assert primary(stride=0) == E and primary(stride=2, offset=2) == E and primary(stride=2, offset=1) == A.RT_OK
    assert primary(h=None) == E and primary(p=None) == E and primary(dp=None) == E and primary(mv=None) == E
    assert primary(h=None, p=None, dp=None, mv=None, n=0) == A.RT_OK
    assert primary(h=hits.ctypes.data + 8) == E and primary(p=paths.ctypes.data + 4) == E
    assert primary(mv=motion.ctypes.data + 4) == E and primary(dp=depth.ctypes.data + 2) == E
    assert primary(mv=motion.ctypes.data + 8, dp=depth.ctypes.data + 4) == A.RT_OK
    assert primary(un=None) == E and primary(scene=None) == E

    rnd = rt.random_offsets(3, W, H)
    rays, pb, extra = np.zeros((W * H * 2 + 1, 8), F), np.zeros((W * H * 2 + 1, 12), F), np.zeros(W * H + 1, np.uint32)

    def extras(un=u, n=W * H, first=0, sample=1, stride=3, rn=rnd.ctypes.data, mv=motion.ctypes.data, pm=None,
               r=rays.ctypes.data, p=pb.ctypes.data, ex=extra.ctypes.data):
        o = A.CameraOpts()
        o.first_pixel, o.sample, o.tag_stride, o.tag_offset = first, sample, stride, 1
        return L.rt_debug_extra_paths_host(C.byref(un) if un is not None else None, C.byref(o), rn, mv, pm, n, r, p, ex)

    assert extras() == A.RT_OK
    assert extras(n=W * H + 1) == E and extras(first=30, n=6) == E and extras(first=30, n=5) == A.RT_OK
    assert extras(sample=-1) == E and extras(stride=0) == E and extras(sample=0x7fffffff) == E
    assert extras(mv=None) == E and extras(ex=None) == E and extras(rn=None) == E and extras(un=None) == E
    assert extras(r=None) == E and extras(p=None) == E           # maxExtra is 2 by default
    assert extras(mv=motion.ctypes.data + 4) == E and extras(pm=motion.ctypes.data + 4) == E and extras(ex=extra.ctypes.data + 2) == E
    assert extras(r=rays.ctypes.data + 8) == E
    off = frame_uniforms(rt, sc, W, H, 0, 1, 2)
    off.enableMotionAdaptiveSampling = 0
    extra[:] = 7
    assert extras(un=off, r=None, p=None) == A.RT_OK             # only `extra` is written
    assert not extra[:W * H].any() and extra[W * H] == 7


def test_primary_hook_selects_records(rt, assets):
    """Dead, bounce > 0, another sample's, a miss, a triangle the scene does not have, a pixel at or
    above `pixels`: none of them writes; the one record that passes does."""
    W, H = 7, 5
    sc = rt.Scene.preset("c1", assets)
    u = frame_uniforms(rt, sc, W, H, 0, 1, 2)
    nt = sc.triangle_count
    stride = 3
    kinds = ["ok", "dead", "bounce", "sample", "miss", "beyond", "pixel"]
    hits, paths = np.zeros((len(kinds), 8), F), np.zeros((len(kinds), 12), F)
    hi, pi = hits.view(np.uint32), paths.view(np.int32)
    hits[:, 0:3] = (2.0, 0.25, 0.5)
    hi[:, 3] = 1
    pi[:, 7] = ALIVE
    pi[:, 11] = np.arange(len(kinds)) * stride                   # pixel k, sample 0
    pi[1, 7] = 0
    pi[2, 8] = 1
    pi[3, 11] += 1
    hi[4, 3] = sr.MISS
    hi[5, 3] = nt
    pi[6, 11] = 20 * stride
    depth, motion = np.full(20, -1.0, F), np.full((20, 2), -1.0, F)
    rt.debug_primary_outputs_host(sc, u, hits, paths, depth, motion, tag_stride=stride)
    assert depth[0] > 0 and np.all(depth[1:] == -1) and np.all(motion[1:] == -1)
    assert np.all(motion[0] == 0)                                # nothing moved
