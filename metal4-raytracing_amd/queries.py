"""Device queries: the record views, the host test hooks and the Renderer's query methods.

Every query (rt_trace_closest / rt_trace_any, rt_resolve_hits, rt_shade_hits, rt_camera_paths,
rt_compact_paths, rt_connect_paths, rt_retire_paths, rt_average_samples) goes through the same
few helpers of RendererQueries: one device record check, one host staging, one `out=` check, one
enqueue.  The six whose record count a compaction produces take `count=`: the count stays on the
device and the call goes to the entry point's _indirect form (rt_device_count).  The temporal
hooks (debug_primary_outputs_host, debug_extra_paths_host, debug_resolve_samples_host) are host
test hooks only: no device query of theirs exists yet.  The package re-exports every public name
of this module.
"""
import ctypes as C

import numpy as np

from . import _abi
from ._abi import CameraOpts, CompactStream, Light, QueryStats


_loaded = None


def _lib():
    global _loaded   # kept: the import statement would cost every query more than its checks do
    if _loaded is None:
        from . import lib
        _loaded = lib()
    return _loaded


def _check(st, ctx=None):
    if st != 0:
        from . import _check as chk
        chk(st, ctx)


def _ptr(x):
    return None if x is None else C.c_void_p(x.data_ptr())


class Hits:
    """Closest-hit results of Renderer.trace: `buffer` holds the (n, 8) rt_ray_hit records and the
    fields are views of it: float32 t (inf on a miss), u, v; int32 triangle, mesh, submesh,
    primitive (-1 on a miss).  Torch tensors on the device path, numpy arrays on the host path."""

    def __init__(self, buffer, as_int):
        self.buffer = buffer
        self.t, self.u, self.v = buffer[:, 0], buffer[:, 1], buffer[:, 2]
        self.triangle, self.mesh, self.submesh, self.primitive = (as_int[:, k] for k in (3, 4, 5, 6))

    def __len__(self):
        return self.buffer.shape[0]


class Surface:
    """Results of Renderer.resolve: `buffer` holds the (n, 16) rt_surface records, `material_buffer`
    the (n, 12) rt_surface_material records (None with material=False), and the fields are views of
    them.  float32: position (n, 3), t, normal (n, 3), uv (n, 2), shading_normal (n, 3) and, with
    materials, base_color (n, 3), opacity, emission (n, 3), ior, roughness, metallic.  int32:
    triangle, mesh, submesh (-1 on a miss), flags (RT_SURFACE_* bits) and, with materials,
    texture_flags, slot.  Torch tensors on the device path, numpy arrays on the host path."""

    HAS_UV, BACKFACE, NORMAL_MAPPED, TRANSMISSIVE = (_abi.RT_SURFACE_HAS_UV, _abi.RT_SURFACE_BACKFACE,
                                                     _abi.RT_SURFACE_NORMAL_MAPPED, _abi.RT_SURFACE_TRANSMISSIVE)

    def __init__(self, buffer, as_int, material_buffer=None, material_as_int=None):
        self.buffer, self.material_buffer = buffer, material_buffer
        self.position, self.t, self.normal = buffer[:, 0:3], buffer[:, 3], buffer[:, 4:7]
        self.uv, self.shading_normal = buffer[:, 7:12:4], buffer[:, 8:11]   # u and v close words 1 and 2
        self.triangle, self.mesh, self.submesh, self.flags = (as_int[:, k] for k in (12, 13, 14, 15))
        if material_buffer is not None:
            m = material_buffer
            self.base_color, self.opacity, self.emission, self.ior = m[:, 0:3], m[:, 3], m[:, 4:7], m[:, 7]
            self.roughness, self.metallic = m[:, 8], m[:, 9]
            self.texture_flags, self.slot = material_as_int[:, 10], material_as_int[:, 11]

    def __len__(self):
        return self.buffer.shape[0]


class Paths:
    """Path states of Renderer.shade: `buffer` holds the (n, 12) rt_path records and the fields are
    views of it.  float32: throughput (n, 3), radiance (n, 3).  int32: sample (the Halton index),
    flags (ALIVE / SHADOW bits), bounce, step, transparency_passes.  Torch tensors on the device
    path, numpy arrays on the host path."""

    ALIVE, SHADOW = _abi.RT_PATH_ALIVE, _abi.RT_PATH_SHADOW

    def __init__(self, buffer, as_int):
        self.buffer = buffer
        self.throughput, self.radiance = buffer[:, 0:3], buffer[:, 4:7]
        self.sample, self.flags = as_int[:, 3], as_int[:, 7]
        self.bounce, self.step, self.transparency_passes = as_int[:, 8], as_int[:, 9], as_int[:, 10]
        self.tag = as_int[:, 11]   # rt_path.reserved: carried through by shade, set by camera_paths, read by retire

    def __len__(self):
        return self.buffer.shape[0]

    @property
    def alive(self):
        return (self.flags & self.ALIVE) != 0

    @property
    def shadow(self):
        return (self.flags & self.SHADOW) != 0


class Shaded:
    """Results of Renderer.shade: `paths` (the Paths given, updated in place), `next_rays` and
    `shadow_rays` ((n, 8) rt_ray records, to trace where paths.alive / paths.shadow) and `contrib`
    ((n, 4): r, g, b, 0; add to paths.radiance where the shadow ray is not occluded)."""

    def __init__(self, paths, next_rays, shadow_rays, contrib):
        self.paths, self.next_rays, self.shadow_rays, self.contrib = paths, next_rays, shadow_rays, contrib

    def __len__(self):
        return len(self.paths)


class Compacted:
    """Results of Renderer.compact: `count` (a 1-element int32 tensor: the number selected),
    `index` (int32, the selected records' positions in ascending order; None when not asked for)
    and `outs` (one full-length tensor per stream; the first `count` records of each are the
    selected ones, the rest is untouched).  n() reads the count back, ordered after the compaction
    on the stream it ran on; slice the tensors with it."""

    def __init__(self, count, index, outs, host, sync):
        self.count, self.index, self.outs = count, index, outs
        self._host, self._sync = host, sync

    def n(self):
        return self._sync(self)


def _shade_opts(shading_mode, max_bounces, light_count):
    o = _abi.ShadeOpts()
    o.shading_mode, o.max_bounces, o.light_count = int(shading_mode), int(max_bounces), int(light_count)
    return o


def _camera_opts(sample, first_pixel, tag_stride, tag_offset):
    o = CameraOpts()
    o.first_pixel, o.sample, o.tag_stride, o.tag_offset = int(first_pixel), int(sample), int(tag_stride), int(tag_offset)
    return o


def debug_trace_host(scene, origins, dirs, tmax=None, any_hit=False):
    """Test hook: trace rays through the library's own BVH + traversal code on the host.
    Returns dict(t, id, u, v, nodes, tris) arrays."""
    o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
    d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
    n = o.shape[0]
    rays = np.ascontiguousarray(np.concatenate([o, d], axis=1), np.float32)
    tm = None if tmax is None else np.ascontiguousarray(np.broadcast_to(tmax, (n,)), np.float32)
    out = dict(t=np.empty(n, np.float32), id=np.empty(n, np.uint32), u=np.empty(n, np.float32),
               v=np.empty(n, np.float32), nodes=np.empty(n, np.uint32), tris=np.empty(n, np.uint32))
    FP, UP = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    d_ = scene.desc()
    _check(_lib().rt_debug_trace_host(C.byref(d_), rays.ctypes.data_as(FP), tm.ctypes.data_as(FP) if tm is not None else None,
                                      n, 1 if any_hit else 0, out["t"].ctypes.data_as(FP), out["id"].ctypes.data_as(UP),
                                      out["u"].ctypes.data_as(FP), out["v"].ctypes.data_as(FP),
                                      out["nodes"].ctypes.data_as(UP), out["tris"].ctypes.data_as(UP)))
    return out


def debug_resolve_host(scene, rays, hits, material=True):
    """Test hook: rt_resolve_hits on the host (rt_debug_resolve_host), over a scene description.
    rays: (n, 8) float32 rt_ray records (Renderer.make_rays); hits: a Hits object or its (n, 8)
    buffer.  Returns a Surface of numpy arrays."""
    r = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
    h = np.ascontiguousarray(hits.buffer if isinstance(hits, Hits) else hits).reshape(-1, 8)
    if h.dtype != np.float32:
        raise ValueError("hits must be float32 (n, 8) rt_ray_hit records")
    n = r.shape[0]
    if h.shape[0] != n:
        raise ValueError(f"{n} rays but {h.shape[0]} hit records")
    surf = np.empty((n, 16), np.float32)
    mat = np.empty((n, 12), np.float32) if material else None
    d_ = scene.desc()
    _check(_lib().rt_debug_resolve_host(C.byref(d_), r.ctypes.data, h.ctypes.data, n, surf.ctypes.data,
                                        mat.ctypes.data if material else None))
    return Surface(surf, surf.view(np.int32), mat, mat.view(np.int32) if material else None)


def debug_shade_host(lights, rays, surface, paths, randoms=None, shading_mode=0, max_bounces=2, light_count=0):
    """Test hook: rt_shade_hits on the host (rt_debug_shade_host) with the given lights (a list of
    Light, or a Scene: its lights).  rays: (n, 8) float32; surface: a Surface with materials (numpy);
    paths: a Paths object or its (n, 12) float32 buffer, NOT modified: the updated copy is
    returned; randoms: None or (n, 8) float32.  Returns a Shaded of numpy arrays."""
    from . import Scene
    if isinstance(lights, Scene):
        d = lights.desc()
        lights = [d.lights[k] for k in range(d.light_count)]
    arr = (Light * max(len(lights), 1))(*lights)
    r = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
    n = r.shape[0]
    if surface.material_buffer is None:
        raise ValueError("shade needs the material records (resolve with material=True)")
    s = np.ascontiguousarray(surface.buffer, np.float32)
    m = np.ascontiguousarray(surface.material_buffer, np.float32)
    pb = paths.buffer if isinstance(paths, Paths) else paths
    if not isinstance(pb, np.ndarray) or pb.dtype != np.float32:
        raise ValueError("paths must be float32 (n, 12) rt_path records")
    p = np.array(pb, np.float32, copy=True, order="C")
    rnd = None if randoms is None else np.ascontiguousarray(randoms, np.float32)
    for name, x, cols in (("surface", s, 16), ("materials", m, 12), ("paths", p, 12), ("randoms", rnd, 8)):
        if x is not None and x.shape != (n, cols):
            raise ValueError(f"{name} must be ({n}, {cols}), not {x.shape}")
    nxt, sh, con = np.empty((n, 8), np.float32), np.empty((n, 8), np.float32), np.empty((n, 4), np.float32)
    o = _shade_opts(shading_mode, max_bounces, light_count)
    _check(_lib().rt_debug_shade_host(arr, len(lights), C.byref(o), r.ctypes.data, s.ctypes.data, m.ctypes.data,
                                      rnd.ctypes.data if rnd is not None else None, n, p.ctypes.data, nxt.ctypes.data,
                                      sh.ctypes.data, con.ctypes.data))
    return Shaded(Paths(p, p.view(np.int32)), nxt, sh, con)


def debug_camera_paths_host(uniforms, random_offsets, sample, first_pixel=0, n=None, tag_stride=1, tag_offset=0):
    """Test hook: rt_camera_paths on the host (rt_debug_camera_paths_host).  random_offsets: the
    width * height uint32 offsets (random_offsets()).  Returns ((n, 8) float32 rays, Paths) as
    numpy arrays; n defaults to the pixels from first_pixel on."""
    rnd = np.ascontiguousarray(random_offsets, np.uint32).reshape(-1)
    if n is None:
        n = max(uniforms.width * uniforms.height - first_pixel, 0)
    if rnd.shape[0] != uniforms.width * uniforms.height:
        raise ValueError(f"random_offsets must hold {uniforms.width * uniforms.height} words, not {rnd.shape[0]}")
    rays, p = np.empty((n, 8), np.float32), np.empty((n, 12), np.float32)
    o = _camera_opts(sample, first_pixel, tag_stride, tag_offset)
    _check(_lib().rt_debug_camera_paths_host(C.byref(uniforms), C.byref(o), rnd.ctypes.data, n, rays.ctypes.data,
                                             p.ctypes.data))
    return rays, Paths(p, p.view(np.int32))


def debug_primary_outputs_host(scene, uniforms, hits, paths, depth, motion, tag_stride=1, tag_offset=0,
                               prev_transforms=None):
    """Test hook rt_debug_primary_outputs_host: depth and motion of sample 0's bounce-0 hits, over a scene
    description whose previous positions are its positions.  hits: a Hits or its (n, 8) float32
    buffer; paths: a Paths or its (n, 12) buffer; depth (pixels elements) and motion (pixels x 2)
    are float32 numpy arrays updated IN PLACE; prev_transforms: (meshes, 4, 3) packed previous
    instance transforms, None = the current ones.  Returns (depth, motion)."""
    h = np.ascontiguousarray(hits.buffer if isinstance(hits, Hits) else hits).reshape(-1, 8)
    pb = paths.buffer if isinstance(paths, Paths) else paths
    p = np.ascontiguousarray(pb).reshape(-1, 12)
    if h.dtype != np.float32 or p.dtype != np.float32 or h.shape[0] != p.shape[0]:
        raise ValueError("hits must be float32 (n, 8) and paths float32 (n, 12) records of one n")
    for name, x, per in (("depth", depth, 1), ("motion", motion, 2)):
        if not (isinstance(x, np.ndarray) and x.dtype == np.float32 and x.flags.c_contiguous and x.size == depth.size * per):
            raise ValueError(f"{name} must be a contiguous float32 array of pixels x {per} elements")
    d_ = scene.desc() if hasattr(scene, "desc") else scene
    pt = None
    if prev_transforms is not None:
        pt = np.ascontiguousarray(prev_transforms, np.float32).reshape(-1, 12)
        if pt.shape[0] != d_.mesh_count:
            raise ValueError(f"{d_.mesh_count} meshes but {pt.shape[0]} previous transforms")
    o = _abi.TargetOpts()
    o.tag_stride, o.tag_offset, o.pixels = int(tag_stride), int(tag_offset), depth.size
    _check(_lib().rt_debug_primary_outputs_host(C.byref(d_), pt.ctypes.data if pt is not None else None, C.byref(uniforms),
                                                C.byref(o), h.ctypes.data, p.ctypes.data, h.shape[0], depth.ctypes.data,
                                                motion.ctypes.data))
    return depth, motion


def debug_extra_paths_host(uniforms, random_offsets, motion, motion_prev=None, sample=None, first_pixel=0, n=None,
                           tag_stride=1, tag_offset=0):
    """Test hook rt_debug_extra_paths_host: the motion-adaptive extra samples.  motion / motion_prev:
    float32 arrays of width * height * 2 elements (motion_prev None = zeros).  Returns ((n *
    maxExtra, 8) rays, Paths, (n,) uint32 extra) as numpy arrays."""
    pixels = uniforms.width * uniforms.height
    rnd = np.ascontiguousarray(random_offsets, np.uint32).reshape(-1)
    if rnd.shape[0] != pixels:
        raise ValueError(f"random_offsets must hold {pixels} words, not {rnd.shape[0]}")
    mv = np.ascontiguousarray(motion, np.float32).reshape(-1)
    pm = None if motion_prev is None else np.ascontiguousarray(motion_prev, np.float32).reshape(-1)
    if mv.shape[0] != 2 * pixels or (pm is not None and pm.shape[0] != 2 * pixels):
        raise ValueError(f"motion targets must hold {pixels} x 2 floats")
    if n is None:
        n = max(pixels - first_pixel, 0)
    me = max(int(uniforms.motionSamplingMaxExtraSamples), 0) if uniforms.enableMotionAdaptiveSampling else 0
    rays, p, extra = np.empty((n * me, 8), np.float32), np.empty((n * me, 12), np.float32), np.empty(n, np.uint32)
    o = _camera_opts(uniforms.samplesPerPixel if sample is None else sample, first_pixel, tag_stride, tag_offset)
    _check(_lib().rt_debug_extra_paths_host(C.byref(uniforms), C.byref(o), rnd.ctypes.data, mv.ctypes.data,
                                            pm.ctypes.data if pm is not None else None, n, rays.ctypes.data, p.ctypes.data,
                                            extra.ctypes.data))
    return rays, Paths(p, p.view(np.int32)), extra


def debug_resolve_samples_host(uniforms, samples, sample_stride, extra=None, motion=None, motion_prev=None, history=None):
    """Test hook rt_debug_resolve_samples_host: the renderer's resolve of any frame.  samples:
    (pixels * sample_stride, 4) float32; extra: (pixels,) uint32 or None; motion, motion_prev:
    pixels x 2 floats or None (zeros); history: pixels x 4 floats, required past frame 0.  Returns
    the (pixels, 4) float32 array."""
    s = np.ascontiguousarray(samples, np.float32).reshape(-1, 4)
    stride = int(sample_stride)
    if stride < 1 or s.shape[0] % stride:
        raise ValueError(f"{s.shape[0]} samples are not a multiple of sample_stride = {stride}")
    pixels = s.shape[0] // stride
    ex = None if extra is None else np.ascontiguousarray(extra, np.uint32).reshape(-1)
    planes = [None if x is None else np.ascontiguousarray(x, np.float32).reshape(-1) for x in (motion, motion_prev, history)]
    for name, x, size in (("extra", ex, pixels), ("motion", planes[0], 2 * pixels), ("motion_prev", planes[1], 2 * pixels),
                          ("history", planes[2], 4 * pixels)):
        if x is not None and x.shape[0] != size:
            raise ValueError(f"{name} must hold {size} elements, not {x.shape[0]}")
    out = np.empty((pixels, 4), np.float32)
    ptr = lambda x: None if x is None else x.ctypes.data
    _check(_lib().rt_debug_resolve_samples_host(C.byref(uniforms), s.ctypes.data, stride, ptr(ex), ptr(planes[0]),
                                                ptr(planes[1]), ptr(planes[2]), pixels, out.ctypes.data))
    return out


class RendererQueries:
    """The query methods of Renderer (a mixin: Renderer inherits it).  Relies on the Renderer's
    self._ctx (the rt_ctx handle), self.device (the HIP device index), self.wait(), self.uniforms()
    and the uniform attributes (width, height, light_count, samplesPerPixel, maxBounces,
    shadingMode).

    A stream argument is a HIP stream handle as in pack_tiles: 0 = HIP's null stream (torch's
    default), None = the renderer's own stream."""

    # --- the one copy of what every query does around its library call ---
    def _device(self):
        """The renderer's torch device, built once."""
        dev = self.__dict__.get("_torch_device")
        if dev is None:
            import torch
            dev = self.__dict__["_torch_device"] = torch.device("cuda", self.device)
        return dev

    def _records(self, x, name, cols, rows=None, dtypes=None):
        """A contiguous tensor on the renderer's device, or ValueError.  cols: an int or the allowed
        widths of 2-D records of 4-byte elements (dtypes: default float32), or None: an int32 vector."""
        import torch
        dev = self._device()
        dtypes = dtypes or ((torch.float32,) if cols is not None else (torch.int32,))
        ok = isinstance(x, torch.Tensor) and x.dtype in dtypes and x.is_contiguous() and x.device == dev
        if ok:
            shape = tuple(x.shape)   # read once: a tensor's attributes are what these checks cost
            ok = (len(shape) == (1 if cols is None else 2) and (rows is None or shape[0] == rows)
                  and (cols is None or shape[1] in ((cols,) if isinstance(cols, int) else cols)))
        if not ok:
            shape = f"({'n' if rows is None else rows},{'' if cols is None else f' {cols}'})"
            raise ValueError(f"{name} must be a contiguous {' / '.join(str(d) for d in dtypes)} {shape} tensor on {dev}")
        return x

    def _words(self, x, name, rows=None):
        """A contiguous int32 vector on the renderer's device, or ValueError."""
        return self._records(x, name, None, rows)

    def _out(self, x, name, rows, cols=None, dtype=None):
        """The caller's `out` tensor checked (_records), or a new one: (rows, cols) of dtype
        (default float32), or with cols None an int32 vector."""
        if x is not None:
            return self._records(x, name, cols, rows, dtype and (dtype,))
        import torch
        if cols is None:
            return torch.empty((rows,), dtype=torch.int32, device=self._device())
        return torch.empty((rows, cols), dtype=dtype or torch.float32, device=self._device())

    def _stage(self, named):
        """Host arrays [(name, array, cols)], each float32 (n, cols) with one n, copied to the device;
        ValueError for a device tensor among them.  Waits once for torch's current stream (the
        copies, and the allocator's stream), since the query runs on another."""
        import torch
        dev = self._device()
        arrays = []
        for name, x, cols in named:
            if isinstance(x, torch.Tensor):
                raise ValueError(f"{named[0][0]} on the host but {name} on the device")
            x = np.ascontiguousarray(x)
            if x.dtype != np.float32 or x.ndim != 2 or x.shape[1] != cols:
                raise ValueError(f"{name} must be float32 (n, {cols}) records")
            if arrays and x.shape[0] != arrays[0].shape[0]:
                raise ValueError(f"{arrays[0].shape[0]} {named[0][0]} but {x.shape[0]} {name} records")
            arrays.append(x)
        staged = [torch.from_numpy(x).to(dev) for x in arrays]
        torch.cuda.current_stream(dev).synchronize()
        return staged

    def _enqueue(self, name, stream, *args, form=""):
        """Calls the entry point `name` on the renderer's stream (stream None) or its `_on` twin
        on `stream`, with the context first; form "_indirect": that entry point's indirect form
        (_n).  Raises RTError on a status."""
        if stream is None:
            _check(getattr(_lib(), name + form)(self._ctx, *args), self._ctx)
        else:
            _check(getattr(_lib(), name + "_on" + form)(self._ctx, *args, C.c_void_p(stream)), self._ctx)

    def _n(self, count, n):
        """The record count of a query as (entry-point suffix, argument): ("", n) for the direct
        form, or with `count` (a 1-element int32 / uint32 tensor on the renderer's device, or a
        Compacted: its .count) ("_indirect", rt_device_count{count, max = n} by reference)."""
        if count is None:
            return "", n
        import torch
        t = count.count if isinstance(count, Compacted) else count
        if not (isinstance(t, torch.Tensor) and t.dtype in (torch.int32, getattr(torch, "uint32", torch.int32))
                and t.numel() == 1 and t.device == self._device()):
            raise ValueError(f"count must be a 1-element int32 / uint32 tensor on {self._device()}, or a Compacted")
        dc = _abi.DeviceCount()
        dc.count, dc.max = t.data_ptr(), n
        return "_indirect", C.byref(dc)

    def _torch_stream(self, stream):
        """The torch stream of a HIP stream handle (0 = torch's default stream)."""
        import torch
        dev = self._device()
        return torch.cuda.default_stream(dev) if not stream else torch.cuda.ExternalStream(stream, device=dev)

    # --- device ray queries (intersector.intersect outside raytracingKernel) ---
    @staticmethod
    def make_rays(origins, dirs, tmax=None):
        """(n, 8) float32 rt_ray records (origin, 0, direction, tmax; tmax None = unbounded) from
        (n, 3) origins and directions: a torch tensor on their device when they are tensors, a
        numpy array otherwise."""
        try:
            import torch
            on_torch = isinstance(origins, torch.Tensor)
        except ImportError:
            on_torch = False
        if on_torch:
            o = origins.reshape(-1, 3).to(torch.float32)
            r = torch.zeros((o.shape[0], 8), dtype=torch.float32, device=o.device)
            r[:, 0:3] = o
            r[:, 4:7] = dirs.reshape(-1, 3).to(torch.float32)
            r[:, 7] = float("inf") if tmax is None else torch.as_tensor(tmax, dtype=torch.float32, device=o.device)
            return r
        o = np.asarray(origins, np.float32).reshape(-1, 3)
        r = np.zeros((o.shape[0], 8), np.float32)
        r[:, 0:3] = o
        r[:, 4:7] = np.asarray(dirs, np.float32).reshape(-1, 3)
        r[:, 7] = np.inf if tmax is None else np.asarray(tmax, np.float32)
        return r

    def trace(self, rays, any_hit=False, out=None, stream=None, count=None):
        """rt_trace_closest / rt_trace_any: traces (n, 8) rays (make_rays) against the geometry the
        next draw() would see.

        Device path: `rays` is a contiguous float32 torch tensor on the renderer's device, read in
        place; the query is enqueued on `stream` without a host wait, and the caller orders `rays`
        (and `out`: (n, 8) float32, or (n,) int32 for any_hit) before that stream.  Returns Hits
        (views of one (n, 8) tensor), or one int32 tensor of 1 / 0 for any_hit.

        Host path: `rays` is a host array (anything that reshapes to (-1, 8)); it is staged through
        torch, the query is waited for and the result comes back as numpy.

        count (here and in resolve, shade, compact, connect and retire; device path only): the
        number of records comes from device memory, a 1-element int32 / uint32 tensor or a
        Compacted (its .count), read when the launch runs: the _indirect entry points.  Only the
        first min(count, n) records are read and written, n being the length of the arrays given;
        outputs come back at full length, the rest of them untouched.  No host wait: the count of
        a compact() on the same stream feeds the next query directly."""
        import torch
        host = not isinstance(rays, torch.Tensor)
        if host and count is not None:
            raise ValueError("count= needs the device path")
        if host:
            r, = self._stage([("rays", np.asarray(rays, np.float32).reshape(-1, 8), 8)])
        else:
            r = self._records(rays, "rays", 8)
        n = r.shape[0]
        out = self._out(out, "out", n, None if any_hit else 8)
        ind, n_arg = self._n(count, n)
        self._enqueue("rt_trace_any" if any_hit else "rt_trace_closest", stream, _ptr(r), n_arg, _ptr(out), form=ind)
        if host:
            self.wait()
            res = out.cpu().numpy()
            return res if any_hit else Hits(res, res.view(np.int32))
        return out if any_hit else Hits(out, out.view(torch.int32))

    def resolve(self, rays, hits, material=True, out=None, stream=None, count=None):
        """rt_resolve_hits: turns (n, 8) rays and their closest-hit records (a Hits object or its
        (n, 8) buffer) into surface and material records: what the renderer itself would shade at
        each hit, bit for bit, against the geometry the next draw() would see.

        Device path (`rays` is a torch tensor; so is the hit buffer): enqueued on `stream` without
        a host wait.  `out` is an (n, 16) float32 tensor, or a pair of it and an (n, 12) one; with
        material=False no material record is written.  Host path (`rays` is a host array): staged
        through torch, waited for, returned as numpy.  count: as in trace.  Returns a Surface."""
        import torch
        hb = hits.buffer if isinstance(hits, Hits) else hits
        host = not isinstance(rays, torch.Tensor)
        if host and count is not None:
            raise ValueError("count= needs the device path")
        if host:
            r, h = self._stage([("rays", np.asarray(rays, np.float32).reshape(-1, 8), 8), ("hits", hb, 8)])
        else:
            r = self._records(rays, "rays", 8)
            h = self._records(hb, "hits", 8, r.shape[0])
        n = r.shape[0]
        surf, mat = (out if isinstance(out, (tuple, list)) else (out, None)) if out is not None else (None, None)
        if mat is not None and not material:
            raise ValueError("a materials tensor was given with material=False")
        surf = self._out(surf, "out surfaces", n, 16)
        mat = self._out(mat, "out materials", n, 12) if material else None
        ind, n_arg = self._n(count, n)
        self._enqueue("rt_resolve_hits", stream, _ptr(r), _ptr(h), n_arg, _ptr(surf), _ptr(mat), form=ind)
        if host:
            self.wait()
            s, m = surf.cpu().numpy(), mat.cpu().numpy() if material else None
            return Surface(s, s.view(np.int32), m, m.view(np.int32) if material else None)
        return Surface(surf, surf.view(torch.int32), mat, mat.view(torch.int32) if material else None)

    @staticmethod
    def make_paths(sample_indices):
        """(n, 12) rt_path records at the camera as a Paths: ALIVE, throughput 1, everything else 0,
        `sample` = the given Halton indices (random offset + frameIndex * stride + sample).  A
        torch tensor on their device when they are a tensor, a numpy array otherwise."""
        try:
            import torch
            on_torch = isinstance(sample_indices, torch.Tensor)
        except ImportError:
            on_torch = False
        if on_torch:
            idx = sample_indices.reshape(-1).to(torch.int64)
            p = torch.zeros((idx.shape[0], 12), dtype=torch.float32, device=idx.device)
            pi = p.view(torch.int32)
            p[:, 0:3] = 1.0
            pi[:, 3] = ((idx + 2 ** 31) % 2 ** 32 - 2 ** 31).to(torch.int32)   # the uint32's bits
            pi[:, 7] = _abi.RT_PATH_ALIVE
            return Paths(p, pi)
        idx = np.asarray(sample_indices).reshape(-1).astype(np.int64)
        p = np.zeros((idx.shape[0], 12), np.float32)
        pu = p.view(np.uint32)
        p[:, 0:3] = 1.0
        pu[:, 3] = idx.astype(np.uint32)
        pu[:, 7] = _abi.RT_PATH_ALIVE
        return Paths(p, p.view(np.int32))

    def shade(self, rays, surface, paths, randoms=None, shading_mode=None, max_bounces=None, light_count=None, out=None,
              stream=None, count=None):
        """rt_shade_hits: what the renderer does between a resolved hit and the next ray.  `rays`
        are the (n, 8) rays that were traced, `surface` their Surface from resolve (with
        materials), `paths` a Paths (make_paths) or its (n, 12) buffer.  Returns a Shaded: the
        paths updated, next_rays to trace where paths.alive, shadow_rays to trace_any where
        paths.shadow, contrib to add to paths.radiance where those are not occluded.
        shading_mode, max_bounces and light_count default to the Renderer's current uniforms;
        randoms: None = the renderer's Halton numbers, or (n, 8) float32 (light, area u, area v,
        glass choice, r0, r1, 0, 0).

        Device path (`rays` is a torch tensor; so are the others): `paths` is updated IN PLACE,
        enqueued on `stream` without a host wait; `out` is a triple of float32 tensors (next_rays
        (n, 8), shadow_rays (n, 8), contrib (n, 4)); next_rays may be `rays`.
        Host path (`rays` is a host array): staged through torch, waited for, returned as numpy;
        the given paths are not modified.  count: as in trace."""
        import torch
        host = not isinstance(rays, torch.Tensor)
        if host and count is not None:
            raise ValueError("count= needs the device path")
        pb = paths.buffer if isinstance(paths, Paths) else paths
        if surface.material_buffer is None:
            raise ValueError("shade needs the material records (resolve with material=True)")
        named = [("rays", rays, 8), ("surface", surface.buffer, 16), ("materials", surface.material_buffer, 12),
                 ("paths", pb, 12)]
        if randoms is not None:
            named.append(("randoms", randoms, 8))
        if host:
            staged = self._stage(named)
        else:
            staged = [self._records(rays, "rays", 8)]
            staged += [self._records(x, name, cols, staged[0].shape[0]) for name, x, cols in named[1:]]
        r, s, m, p = staged[:4]
        rnd = staged[4] if randoms is not None else None
        n = r.shape[0]
        if out is not None and (not isinstance(out, (tuple, list)) or len(out) != 3):
            raise ValueError("out must be (next_rays, shadow_rays, contrib)")
        outs = [self._out(out[k] if out is not None else None, "out " + name, n, cols)
                for k, (name, cols) in enumerate((("next_rays", 8), ("shadow_rays", 8), ("contrib", 4)))]
        o = _shade_opts(self.shadingMode if shading_mode is None else shading_mode,
                        self.maxBounces if max_bounces is None else max_bounces,
                        self.light_count if light_count is None else light_count)
        ind, n_arg = self._n(count, n)
        self._enqueue("rt_shade_hits", stream, C.byref(o), _ptr(r), _ptr(s), _ptr(m), _ptr(rnd), n_arg, _ptr(p),
                      _ptr(outs[0]), _ptr(outs[1]), _ptr(outs[2]), form=ind)
        if host:
            self.wait()
            pn = p.cpu().numpy()
            return Shaded(Paths(pn, pn.view(np.int32)), *(x.cpu().numpy() for x in outs))
        return Shaded(paths if isinstance(paths, Paths) else Paths(p, p.view(torch.int32)), *outs)

    # --- path queries: the glue of a query integrator as library calls ---
    def camera_paths(self, sample, first_pixel=0, n=None, uniforms=None, random_offsets=None, tag_stride=1, tag_offset=0,
                     out=None, stream=None):
        """rt_camera_paths: the renderer's primary rays and path states of sample `sample` for the n
        pixels from first_pixel on (row-major; default: the rest of the image), by the given
        uniforms (default: the Renderer's current ones: camera, size, frameIndex, samplesPerPixel).
        random_offsets: None = the renderer's own, or width * height offsets as an int32 tensor on
        the device (a host array is staged).  Each path's tag is pixel * tag_stride + tag_offset.
        `out` is a pair of float32 tensors ((n, 8) rays, (n, 12) paths).  Enqueued on `stream`
        without a host wait.  Returns (rays, Paths)."""
        import torch
        u = uniforms if uniforms is not None else self.uniforms()
        if n is None:
            n = u.width * u.height - int(first_pixel)
        if n < 0:
            raise ValueError("first_pixel is past the image")
        rnd = random_offsets
        if rnd is not None:
            if not isinstance(rnd, torch.Tensor):   # staged as the words' float32 bits: a copy does not read them
                bits = np.ascontiguousarray(rnd, np.uint32).reshape(-1, 1).view(np.float32)
                rnd = self._stage([("random_offsets", bits, 1)])[0].view(torch.int32).reshape(-1)
            self._words(rnd, "random_offsets", u.width * u.height)
        if out is not None and (not isinstance(out, (tuple, list)) or len(out) != 2):
            raise ValueError("out must be (rays, paths)")
        rays = self._out(out[0] if out is not None else None, "out rays", n, 8)
        pb = self._out(out[1] if out is not None else None, "out paths", n, 12)
        o = _camera_opts(sample, first_pixel, tag_stride, tag_offset)
        self._enqueue("rt_camera_paths", stream, C.byref(u), C.byref(o), _ptr(rnd), n, _ptr(rays), _ptr(pb))
        return rays, Paths(pb, pb.view(torch.int32))

    def compact(self, paths, mask, streams=(), index=True, out=None, stream=None, count=None):
        """rt_compact_paths: stable compaction of up to four record streams by the paths' flags:
        the records i with paths.flags[i] & mask != 0, in ascending i, what x[(flags & mask) != 0]
        gives.  `paths` is a Paths or its (n, 12) buffer; `streams` are (n, 4 * words) tensors of
        4-byte elements, words 1 .. 4 (the paths buffer itself may be one).  index: True = also
        return the selected positions, False = not, or an int32 (n,) tensor to write them to.
        out: a Compacted of an earlier call of the same shapes, or a tuple (outs, index, count) of
        tensors to write to (outs: one per stream, same shape and type; index / count may be None).
        Not in place: no output may be an input.  Enqueued on `stream` without a host wait;
        Compacted.n() reads the count back.  count: as in trace, the records compacted are the
        first min(count, n); the count written is always a word of its own (RTError otherwise),
        and it is written whenever n > 0, so it can be the next query's count."""
        import torch
        four = (torch.float32, torch.int32)
        count_in = count
        pb = self._records(paths.buffer if isinstance(paths, Paths) else paths, "paths", 12)
        n = pb.shape[0]
        srcs = [self._records(x, f"stream {k}", (4, 8, 12, 16), n, four) for k, x in enumerate(streams)]
        if len(srcs) > 4:
            raise ValueError("at most four streams")
        o_outs = o_index = o_count = host = None
        if isinstance(out, Compacted):
            o_outs, o_index, o_count, host = out.outs, out.index, out.count, out._host
        elif out is not None:
            if not isinstance(out, (tuple, list)) or len(out) != 3:
                raise ValueError("out must be a Compacted or (outs, index, count)")
            o_outs, o_index, o_count = out
        if o_outs is not None and len(o_outs) != len(srcs):
            raise ValueError(f"{len(srcs)} streams but {len(o_outs)} out tensors")
        outs = [self._out(o_outs[k] if o_outs is not None else None, f"out {k}", n, x.shape[1], x.dtype)
                for k, x in enumerate(srcs)]
        if isinstance(index, torch.Tensor):
            idx = self._words(index, "index", n)
        else:
            idx = self._out(o_index, "out index", n) if index else None
        count = self._out(o_count, "out count", 1)
        if host is None:
            host = torch.empty((1,), dtype=torch.int32, pin_memory=True)
        arr = (CompactStream * max(len(srcs), 1))()
        for k, (x, d) in enumerate(zip(srcs, outs)):
            arr[k].src, arr[k].dst, arr[k].words = x.data_ptr(), d.data_ptr(), x.shape[1] // 4
        if n == 0:   # nothing is launched and nothing written: the count is ours to set
            with torch.cuda.stream(self._torch_stream(stream) if stream is not None
                                   else torch.cuda.current_stream(self._device())):
                count.zero_()
        ind, n_arg = self._n(count_in, n)
        self._enqueue("rt_compact_paths", stream, _ptr(pb), n_arg, int(mask), arr, len(srcs), _ptr(idx), _ptr(count),
                      form=ind)

        def sync(cp, stream=stream):
            if stream is None:
                self.wait()   # the renderer's own stream is not torch's to name
                cp._host.copy_(cp.count)
            else:
                ts = self._torch_stream(stream)
                with torch.cuda.stream(ts):
                    cp._host.copy_(cp.count, non_blocking=True)
                ts.synchronize()
            return int(cp._host[0])

        return Compacted(count, idx, outs, host, sync)

    def connect(self, paths, contrib, occluded, index=None, m=None, stream=None, count=None):
        """rt_connect_paths: paths.radiance[i] += contrib[i] for the first m shadow rays j that
        are not occluded (occluded[j] == 0), i = index[j] (or j without an index).  `paths`
        (Paths or buffer) is updated IN PLACE; contrib is (n, 4) float32, occluded and index int32
        vectors of at least m entries (m defaults to len(occluded)).  The index entries must be
        distinct, as compact() makes them.  Enqueued on `stream` without a host wait.  count: as in
        trace, the number of shadow rays (m, then their bound) from device memory."""
        pb = self._records(paths.buffer if isinstance(paths, Paths) else paths, "paths", 12)
        n = pb.shape[0]
        con = self._records(contrib, "contrib", 4, n)
        occ = self._words(occluded, "occluded")
        idx = self._words(index, "index") if index is not None else None
        m = occ.shape[0] if m is None else int(m)
        if m < 0 or m > occ.shape[0] or (idx is not None and m > idx.shape[0]):
            raise ValueError(f"m = {m} is more than occluded / index hold")
        ind, m_arg = self._n(count, m)
        self._enqueue("rt_connect_paths", stream, _ptr(pb), n, _ptr(con), _ptr(idx), _ptr(occ), m_arg, form=ind)

    def retire(self, paths, samples, stream=None, count=None):
        """rt_retire_paths: samples[tag] = (radiance, 1) for every path that is not ALIVE and whose
        tag is below len(samples); `samples` is a (tags, 4) float32 tensor.  Enqueued on `stream`
        without a host wait.  count: as in trace."""
        pb = self._records(paths.buffer if isinstance(paths, Paths) else paths, "paths", 12)
        sm = self._records(samples, "samples", 4)
        ind, n_arg = self._n(count, pb.shape[0])
        self._enqueue("rt_retire_paths", stream, _ptr(pb), n_arg, _ptr(sm), sm.shape[0], form=ind)

    def average(self, samples, spp, out=None, stream=None):
        """rt_average_samples: (pixels * spp, 4) float32 samples, a pixel's spp samples side by
        side, into (pixels, 4): their sum in sample order / spp, alpha 1, as the renderer resolves
        frame 0.  Enqueued on `stream` without a host wait.  Returns the (pixels, 4) tensor."""
        sm = self._records(samples, "samples", 4)
        spp = int(spp)
        if spp < 1 or sm.shape[0] % spp:
            raise ValueError(f"{sm.shape[0]} samples are not a multiple of spp = {spp}")
        pixels = sm.shape[0] // spp
        out = self._out(out, "out", pixels, 4)
        self._enqueue("rt_average_samples", stream, _ptr(sm), pixels, spp, _ptr(out))
        return out

    def _path_buffers(self, cap, tags):
        """path_trace's working set, allocated once per size: two sets of rays and paths to
        ping-pong between, one of everything else."""
        import torch
        have = self.__dict__.get("_pt_buffers")
        if have is not None and have["cap"] == cap and have["tags"] == tags:
            return have
        dev = self._device()
        f = lambda cols, rows=cap: torch.empty((rows, cols), dtype=torch.float32, device=dev)
        w = lambda rows=cap: torch.empty((rows,), dtype=torch.int32, device=dev)
        pin = lambda: torch.empty((1,), dtype=torch.int32, pin_memory=True)
        b = dict(cap=cap, tags=tags, rays=[f(8), f(8)], paths=[f(12), f(12)], hits=f(8), surf=f(16), mat=f(12), nxt=f(8),
                 shadow=f(8), contrib=f(4), shadow_c=f(8), sh_index=w(), occluded=w(), samples=f(4, tags),
                 counts=[w(1), w(1)], pinned=[pin(), pin()])
        self._pt_buffers = b
        return b

    def _device_rounds(self, B, guard, lookahead, mode, mb, stream, ts):
        """path_trace's rounds over one group of camera paths with every count on the device.
        B["words"] is two (alive, shadow) pairs: round r reads its alive count from pair `cur` and
        writes the next alive count and its shadow count into the other pair, which one 8-byte
        copy then takes to row r of the pinned B["rows"], followed by event r.  Before round r is
        enqueued the host waits for event r - 1 - lookahead and reads that row: alive 0 ends the
        loop (the rounds enqueued past it ran on count 0 and changed nothing), anything else is
        the new host bound of the arrays (counts never grow).  Returns (closest rays, shadow rays,
        rounds that had a count, host waits)."""
        import torch
        A, SH = Paths.ALIVE, Paths.SHADOW
        W, rows, events = B["words"], B["rows"], B["events"]
        q = dict(stream=stream)
        n = B["cap"]
        with torch.cuda.stream(ts):
            W[0, 0:1].fill_(n)
        cur, r, closest, shadows = 0, 0, n, 0
        while True:
            j = r - 1 - lookahead
            if j >= 0:
                events[j].synchronize()
                alive, ns = int(rows[j, 0]), int(rows[j, 1])
                shadows += ns
                if alive == 0:
                    return closest, shadows, j + 1, j + 1
                if j + 1 >= guard:
                    raise RuntimeError(f"a path outlived the renderer's longest ({guard} steps)")
                closest += alive
                n = alive
            c_in, c_alive, c_shadow = W[cur, 0:1], W[1 - cur, 0:1], W[1 - cur, 1:2]
            rays, pb = B["rays"][cur][:n], B["paths"][cur][:n]
            nxt, shadow, contrib = B["nxt"][:n], B["shadow"][:n], B["contrib"][:n]
            hits = self.trace(rays, out=B["hits"][:n], count=c_in, **q)
            S = self.resolve(rays, hits, out=(B["surf"][:n], B["mat"][:n]), count=c_in, **q)
            self.shade(rays, S, pb, shading_mode=mode, max_bounces=mb, out=(nxt, shadow, contrib), count=c_in, **q)
            self.compact(pb, SH, (shadow,), out=Compacted(c_shadow, B["sh_index"][:n], [B["shadow_c"][:n]], B["pinned"][0], None),
                         count=c_in, **q)
            self.trace(B["shadow_c"][:n], any_hit=True, out=B["occluded"][:n], count=c_shadow, **q)
            self.connect(pb, contrib, B["occluded"][:n], index=B["sh_index"][:n], m=n, count=c_shadow, **q)
            self.retire(pb, B["samples"], count=c_in, **q)
            self.compact(pb, A, (nxt, pb), index=False,
                         out=Compacted(c_alive, None, [B["rays"][1 - cur][:n], B["paths"][1 - cur][:n]], B["pinned"][1],
                                       None),
                         count=c_in, **q)
            with torch.cuda.stream(ts):
                rows[r].copy_(W[1 - cur], non_blocking=True)
            events[r].record(ts)
            cur, r = 1 - cur, r + 1

    def path_trace(self, spp=None, max_bounces=None, shading_mode=None, stream=0, batch_samples=True, device_counts=False,
                   lookahead=1):
        """Frame 0 of the current uniforms from queries only: camera_paths, then per round
        trace -> resolve -> shade -> compact(SHADOW: shadow rays + index) -> trace(any_hit) ->
        connect -> retire -> compact(ALIVE: next rays + paths) until no path is left, then
        average.  Bit-identical to draw() + radiance() of frame 0 in all four channels.  The host's
        part per round is reading the two compactions' counts.  batch_samples: all samples of the
        image in one array (tag = pixel * spp + s), else one sample at a time.  Runs on `stream`
        (default 0 = torch's default stream); the working buffers are allocated once per size and
        kept.  Returns the (H, W, 4) float32 tensor, valid on that stream; the ray totals are kept
        in `last_path_trace` (closest_rays, shadow_rays, paths, rounds).

        device_counts=True runs the same rounds through the count= forms: every launch takes its
        count from the device, sized on the host by the newest alive count the host has seen, and
        per round one 8-byte copy of (alive, shadow) and one event go to the host.  The host waits
        for the event of round r - 1 - lookahead before it enqueues round r, and stops when that
        round left no path: `lookahead` rounds are in flight beyond the one waited for, and at the
        end as many run on a count of 0.  lookahead=0 waits once per round.  Needs a stream torch
        can name (not None).  Same image, same totals; last_path_trace gains host_waits (event
        waits; as `rounds`, of the group of samples that took the most)."""
        import torch
        dev = self._device()
        lookahead = int(lookahead)
        if device_counts and (stream is None or lookahead < 0):
            raise ValueError("device_counts needs a stream handle (0 = torch's default) and lookahead >= 0")
        spp = int(self.samplesPerPixel if spp is None else spp)
        mb = int(self.maxBounces if max_bounces is None else max_bounces)
        mode = int(self.shadingMode if shading_mode is None else shading_mode)
        if spp < 1 or spp > 64:
            raise ValueError("spp outside 1 .. 64")
        u = self.uniforms()
        u.frameIndex, u.samplesPerPixel = 0, spp
        pixels = self.width * self.height
        guard = mb * (mb + 1) + 1   # shade steps a path can take at most (tests/shade_ref.py guard_steps)
        ts = self._torch_stream(stream) if stream is not None else None
        with torch.cuda.stream(ts if ts is not None else torch.cuda.current_stream(dev)):
            B = self._path_buffers(pixels * spp if batch_samples else pixels, pixels * spp)
            image = torch.empty((pixels, 4), dtype=torch.float32, device=dev)
            if device_counts and (B.get("rows") is None or B["rows"].shape[0] != guard + lookahead):
                B["words"] = torch.zeros((2, 2), dtype=torch.int32, device=dev)
                B["rows"] = torch.zeros((guard + lookahead, 2), dtype=torch.int32, pin_memory=True)
                B["events"] = [torch.cuda.Event() for _ in range(guard + lookahead)]
        A, SH = Paths.ALIVE, Paths.SHADOW
        q = dict(stream=stream)
        totals = dict(closest_rays=0, shadow_rays=0, paths=pixels * spp, rounds=0)
        for group in ([range(spp)] if batch_samples else [[s] for s in range(spp)]):
            cur = 0
            for s in group:
                k = s * pixels if batch_samples else 0
                self.camera_paths(s, uniforms=u, tag_stride=spp, tag_offset=s,
                                  out=(B["rays"][cur][k:k + pixels], B["paths"][cur][k:k + pixels]), **q)
            if device_counts:
                nc, ns, rounds, waits = self._device_rounds(B, guard, lookahead, mode, mb, stream, ts)
                totals["closest_rays"] += nc
                totals["shadow_rays"] += ns
                totals["rounds"] = max(totals["rounds"], rounds)
                totals["host_waits"] = max(totals.get("host_waits", 0), waits)
                continue
            n, rounds = B["cap"], 0
            while n > 0:
                if rounds >= guard:
                    raise RuntimeError(f"a path outlived the renderer's longest ({guard} steps)")
                rays, pb = B["rays"][cur][:n], B["paths"][cur][:n]
                nxt, shadow, contrib = B["nxt"][:n], B["shadow"][:n], B["contrib"][:n]
                hits = self.trace(rays, out=B["hits"][:n], **q)
                S = self.resolve(rays, hits, out=(B["surf"][:n], B["mat"][:n]), **q)
                self.shade(rays, S, pb, shading_mode=mode, max_bounces=mb, out=(nxt, shadow, contrib), **q)
                ns = self.compact(pb, SH, (shadow,), out=Compacted(B["counts"][0], B["sh_index"][:n], [B["shadow_c"][:n]],
                                                                    B["pinned"][0], None), **q).n()
                if ns:
                    self.trace(B["shadow_c"][:ns], any_hit=True, out=B["occluded"][:ns], **q)
                    self.connect(pb, contrib, B["occluded"][:ns], index=B["sh_index"][:ns], m=ns, **q)
                self.retire(pb, B["samples"], **q)
                na = self.compact(pb, A, (nxt, pb), index=False,
                                  out=Compacted(B["counts"][1], None, [B["rays"][1 - cur][:n], B["paths"][1 - cur][:n]],
                                                B["pinned"][1], None), **q).n()
                totals["closest_rays"] += n
                totals["shadow_rays"] += ns
                n, cur, rounds = na, 1 - cur, rounds + 1
            totals["rounds"] = max(totals["rounds"], rounds)
        self.average(B["samples"], spp, out=image, **q)
        if stream is None:
            self.wait()
        self.last_path_trace = totals
        return image.view(self.height, self.width, 4)

    def query_stats(self):
        """rt_get_query_stats (waits for pending queries): the last query and the running totals."""
        s = QueryStats()
        _check(_lib().rt_get_query_stats(self._ctx, C.byref(s)), self._ctx)
        return s
