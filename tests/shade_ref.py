"""Shared by tests/test_shade_host.py and tests/test_gpu_shade.py (no tests here): the camera rays
and Halton indices of one sample of frame 0, and the renderer's path tracer re-assembled from
queries (trace -> resolve -> shade -> trace_any + trace -> ...), written once over a small backend
interface so the host hooks and the device queries run the same loop.  Every comparison made with
these is bitwise."""
import os

import numpy as np

import surface_ref as sr

F = np.float32
MISS = sr.MISS
ALIVE, SHADOW = 1, 2
# (t = inf, u = v = 0, triangle = mesh = submesh = primitive = MISS, 0): rq_trace's miss record
MISS_HIT = np.array([sr.INF_BITS, 0, 0, MISS, MISS, MISS, MISS, 0], np.uint32)
# the three output records of a path that was not shaded, or of a step without the ray
ZERO_RAY = np.array([0, 0, 0, 0, 0, 0, 0, -1], F)


def guard_steps(max_bounces):
    """Shade steps a path can take at most: every bounce may be preceded by max_bounces
    transparency passes (the pass after those consumes the bounce)."""
    return max_bounces * (max_bounces + 1) + 1


def sample_rays(rt, orc, W, H, seed, s=0, camera=None):
    """Sample s's primary rays of frame 0, pixel by pixel in row-major order, as primary_ray
    (csrc/rt_shade.h) forms them, and their Halton indices (random offset + s; frameIndex = 0):
    surface_ref.camera_rays generalised to offset + s.  Returns (origins, directions, indices)."""
    rnd = rt.random_offsets(seed, W, H)
    idx = rnd.astype(np.int64) + s
    cam = camera if camera is not None else rt.camera_default(W, H)
    rx = np.array([orc.halton(int(i), 0) for i in idx], F)
    ry = np.array([orc.halton(int(i), 1) for i in idx], F)
    px = np.tile(np.arange(W, dtype=F), H)
    py = np.repeat(np.arange(H, dtype=F), W)
    uvx = (px + rx) / F(W)
    uvy = (py + ry) / F(H)
    uvx = uvx * F(2) - F(1)
    uvy = uvy * F(2) - F(1)
    d = (uvx[:, None] * sr._v3(cam.right) + uvy[:, None] * sr._v3(cam.up)) + sr._v3(cam.forward)
    d = sr._normalize(d)
    o = np.broadcast_to(sr._v3(cam.position), d.shape).copy()
    return o, np.ascontiguousarray(d, F), idx


def glass_scene(rt, assets):
    """c1 plus the teapot (15,704 triangles) in glass at the presets' hero position, and a small
    near-black sphere beside it.  The sphere is what ends paths on the throughput cut-off
    (length(color) < 1e-3, :751-753): c1's darkest material is the floor's 0.5, and 0.5^8 * sqrt(3)
    = 6.8e-3 stays above it within 8 bounces; glass hits never take that branch."""
    sc = rt.Scene.preset("c1", assets)
    sc.add_model(os.path.join(assets, "teapot.obj"), GLASS_POS, scale=GLASS_SCALE, material_override=rt.glass_override())
    dark = rt.MaterialOverride()
    dark.has_base_color = 1
    dark.base_color[:] = (4e-4, 4e-4, 4e-4)
    sc.add_model(os.path.join(assets, "sphere.obj"), DARK_POS, scale=DARK_SCALE, material_override=dark)
    return sc


GLASS_POS, GLASS_SCALE = (0.3, 0.38, 2.5), 0.004
DARK_POS, DARK_SCALE = (-0.6, 0.0, 2.2), 0.3


def scene_lights(scene):
    """Copies of the scene's lights (the descriptor points into the scene, which may change)."""
    d = scene.desc()
    return [type(d.lights[k]).from_buffer_copy(d.lights[k]) for k in range(d.light_count)]


# ---- backends: trace(rays) -> (n, 8) hit records; trace_any(rays) -> occluded (n,), nonzero = hit;
# resolve(rays, hits) -> Surface; shade(rays, surface, paths) -> Shaded; plus the few array
# operations the loop needs.  Rays, hits and paths are (n, 8) / (n, 8) / (n, 12) float32 buffers.
class HostBackend:
    """debug_trace_host / debug_resolve_host / debug_shade_host over a scene, numpy arrays."""

    def __init__(self, rt, scene, shading_mode, max_bounces, light_count=0):
        self.rt, self.scene = rt, scene
        self.lights = scene_lights(scene)
        self.opts = dict(shading_mode=shading_mode, max_bounces=max_bounces, light_count=light_count)

    def trace(self, rays):
        return sr.hit_records(self.rt.debug_trace_host(self.scene, rays[:, 0:3], rays[:, 4:7]))

    def trace_any(self, rays):
        return self.rt.debug_trace_host(self.scene, rays[:, 0:3], rays[:, 4:7], tmax=rays[:, 7], any_hit=True)["id"] != MISS

    def resolve(self, rays, hits):
        return self.rt.debug_resolve_host(self.scene, rays, hits)

    def shade(self, rays, surface, paths, randoms=None):
        return self.rt.debug_shade_host(self.lights, rays, surface, paths, randoms=randoms, **self.opts)

    def miss_hits(self, n):
        return np.broadcast_to(MISS_HIT.view(F), (n, 8)).copy()

    def paths(self, buffer):
        return self.rt.Paths(buffer, buffer.view(np.int32))

    zeros = staticmethod(lambda shape: np.zeros(shape, F))
    arange = staticmethod(lambda n: np.arange(n))
    where = staticmethod(np.where)
    count = staticmethod(lambda mask: int(mask.sum()))
    numpy = staticmethod(lambda x: x)


class DeviceBackend:
    """Renderer.trace / resolve / shade with torch tensors, everything on one stream (HIP's null
    stream, torch's default: each step is ordered after the one before)."""

    def __init__(self, rt, R, stream=0):
        import torch
        self.rt, self.R, self.torch, self.stream = rt, R, torch, stream
        self.dev = torch.device("cuda", R.device)

    def trace(self, rays):
        return self.R.trace(rays, stream=self.stream).buffer

    def trace_any(self, rays):
        return self.R.trace(rays, any_hit=True, stream=self.stream)

    def resolve(self, rays, hits):
        return self.R.resolve(rays, hits, stream=self.stream)

    def shade(self, rays, surface, paths, randoms=None):
        return self.R.shade(rays, surface, paths, randoms=randoms, stream=self.stream)

    def miss_hits(self, n):
        return self.torch.from_numpy(MISS_HIT.view(F)).to(self.dev).expand(n, 8).contiguous()

    def paths(self, buffer):
        return self.rt.Paths(buffer, buffer.view(self.torch.int32))

    def zeros(self, shape):
        return self.torch.zeros(shape, dtype=self.torch.float32, device=self.dev)

    def arange(self, n):
        return self.torch.arange(n, device=self.dev)

    def where(self, c, a, b):
        return self.torch.where(c, a, b)

    def count(self, mask):
        return int(mask.sum().item())

    def numpy(self, x):
        return x.cpu().numpy()


def integrate(B, rays, paths, max_bounces, compact, record=None):
    """The renderer's bounce loop over one sample's paths, from queries.  Until no path is ALIVE:
    trace -> resolve -> shade; trace_any the SHADOW records' shadow rays (boolean-index
    compaction); radiance += contrib where unoccluded; the rays become next_rays.  compact = True
    drops the dead records before every trace; False carries them (their hit records are misses,
    shade leaves them alone).  record(rays, surface, paths) sees every shade call's inputs.
    Returns (radiance (n, 3) in the order given, closest rays traced, shadow rays traced,
    paths object at the end (carry form: every record))."""
    n = len(paths)
    index = B.arange(n)
    radiance = B.zeros((n, 3))
    closest = shadow = 0
    for it in range(guard_steps(max_bounces) + 1):
        alive = paths.alive
        na = B.count(alive)
        if na == 0:
            break
        assert it < guard_steps(max_bounces), "a path outlived the renderer's longest"
        if compact:
            radiance[index[~alive]] = paths.radiance[~alive]
            rays, index, paths = rays[alive], index[alive], B.paths(paths.buffer[alive])
            hits = B.trace(rays)
        else:
            hits = B.miss_hits(n)
            hits[alive] = B.trace(rays[alive])
        closest += na
        S = B.resolve(rays, hits)
        if record is not None:
            record(rays, S, paths)
        out = B.shade(rays, S, paths)
        paths = out.paths
        sh = paths.shadow
        ns = B.count(sh)
        if ns:
            occluded = B.trace_any(out.shadow_rays[sh])
            lit = sh.copy() if isinstance(sh, np.ndarray) else sh.clone()
            lit[sh] = occluded == 0
            paths.radiance[:] = B.where(lit[:, None], paths.radiance + out.contrib[:, 0:3], paths.radiance)
        shadow += ns
        rays = out.next_rays
    radiance[index] = paths.radiance
    return radiance, closest, shadow, paths


def render(B, rt, orc, W, H, seed, spp, max_bounces, compact, to_backend=lambda x: x, record=None, ends=None):
    """Frame 0 from queries: per sample s the camera rays and integrate(), then pixel = (sum of the
    samples' radiance in sample order) / spp in float32 (:777, :792).  to_backend moves the numpy
    rays and path buffers to the backend's arrays; ends collects every sample's final paths.
    Returns dict(radiance (H, W, 3) numpy, closest_rays, shadow_rays, paths)."""
    total = None
    closest = shadow = 0
    for s in range(spp):
        o, d, idx = sample_rays(rt, orc, W, H, seed, s)
        rays = to_backend(rt.Renderer.make_rays(o, d))
        paths = B.paths(to_backend(rt.Renderer.make_paths(idx).buffer))
        rad, nc, ns, end = integrate(B, rays, paths, max_bounces, compact, record)
        rad = B.numpy(rad)
        total = rad if total is None else total + rad
        closest += nc
        shadow += ns
        if ends is not None:
            ends.append(end)
    return dict(radiance=(total / F(spp)).reshape(H, W, 3), closest_rays=closest, shadow_rays=shadow, paths=W * H * spp)
