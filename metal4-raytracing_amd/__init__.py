"""metal4-raytracing_amd — MI355X-native path tracer for the raytracingKernel hot path.

Python host mirror of the reference's Swift interface for this path, over the C-ABI
library librt_hip.so (include/rt_api.h, include/rt_scene.h):

    Scene      ~ MetalRaytracing/Scene.swift + AppScene.swift (models, lights, orbit camera)
    Renderer   ~ MetalRaytracing/Renderer.swift (knobs with didSet -> frameIndex = 0,
                 updateUniforms, draw, accumulation ping-pong)

The compute path is the HIP library; there is no CPU fallback: importing this package on a
machine without the built library raises, and Renderer() raises without a HIP device.
Load it with importlib.import_module("metal4-raytracing_amd") (the directory name has a dash).
"""
import ctypes as C
import os

import numpy as np

from . import _abi
from ._abi import (TEXTURE_SLOTS, Tuning, Camera, Float3, Light, MaterialOverride, PackedFloat4x3, SceneDesc, Stats, TextureDesc,
                   TileSet, Uniforms, Ray, RayHit, QueryStats, Path, ShadeOpts, CameraOpts, CompactStream,
                   f3)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "librt_hip.so")
ASSET_DIR_DEFAULT = os.environ.get("RT_ASSET_DIR", os.path.join(os.path.dirname(_HERE), "assets"))

_lib = None


class RTError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"rt status {code}: {msg}")
        self.code = code


def lib():
    """The loaded librt_hip.so (raises if it was not built — no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing: run __graft_entry__.build() (make -C metal4-raytracing_amd)")
        # torch bundles its own libamdhip64.so.7 (same soname as /opt/rocm's). Load torch first so
        # the process holds ONE HIP runtime; torch.distributed / tensors then share it with us.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        _lib = _abi.declare(C.CDLL(LIB_PATH))
    return _lib


def _check(st, ctx=None, scene=None):
    if st != 0:
        if scene is not None:
            msg = lib().rt_scene_last_error(scene)
        else:
            msg = lib().rt_last_error(ctx)
        raise RTError(st, (msg or b"").decode())


def version():
    return lib().rt_version().decode()


def uniforms_default(width, height, light_count=2):
    u = Uniforms()
    lib().rt_uniforms_default(width, height, light_count, C.byref(u))
    return u


def decode_png(data):
    """PNG bytes -> (H, W, 4) uint8 RGBA (row 0 = top), the library's texture decoder."""
    buf = (C.c_uint8 * len(data)).from_buffer_copy(data)
    w, h = C.c_uint32(0), C.c_uint32(0)
    err = C.create_string_buffer(256)
    st = lib().rt_decode_png(buf, len(data), None, C.byref(w), C.byref(h), err, 256)
    if st != 0:
        raise RTError(st, err.value.decode())
    out = np.empty((h.value, w.value, 4), dtype=np.uint8)
    st = lib().rt_decode_png(buf, len(data), out.ctypes.data, C.byref(w), C.byref(h), err, 256)
    if st != 0:
        raise RTError(st, err.value.decode())
    return out


def write_png(path, rgba8):
    """(H, W, 4) uint8 rows top-down -> an RGBA PNG file (e.g. Renderer.present())."""
    a = np.ascontiguousarray(rgba8, dtype=np.uint8)
    assert a.ndim == 3 and a.shape[2] == 4, a.shape
    _check(lib().rt_write_png(str(path).encode(), a.ctypes.data, a.shape[1], a.shape[0]))


def camera_default(width, height):
    c = Camera()
    lib().rt_camera_default(width, height, C.byref(c))
    return c


def random_offsets(seed, width, height):
    """splitmix64(seed) % 2^20 per pixel, row-major (Renderer.swift:719-738, seeded)."""
    out = np.empty(width * height, dtype=np.uint32)
    lib().rt_random_offsets(seed, width, height, out.ctypes.data_as(C.POINTER(C.c_uint32)))
    return out


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
    _check(lib().rt_debug_trace_host(C.byref(d_), rays.ctypes.data_as(FP), tm.ctypes.data_as(FP) if tm is not None else None,
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
    _check(lib().rt_debug_resolve_host(C.byref(d_), r.ctypes.data, h.ctypes.data, n, surf.ctypes.data,
                                       mat.ctypes.data if material else None))
    return Surface(surf, surf.view(np.int32), mat, mat.view(np.int32) if material else None)


def debug_shade_host(lights, rays, surface, paths, randoms=None, shading_mode=0, max_bounces=2, light_count=0):
    """Test hook: rt_shade_hits on the host (rt_debug_shade_host) with the given lights (a list of
    Light, or a Scene: its lights).  rays: (n, 8) float32; surface: a Surface with materials (numpy);
    paths: a Paths object or its (n, 12) float32 buffer, NOT modified: the updated copy is
    returned; randoms: None or (n, 8) float32.  Returns a Shaded of numpy arrays."""
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
    _check(lib().rt_debug_shade_host(arr, len(lights), C.byref(o), r.ctypes.data, s.ctypes.data, m.ctypes.data,
                                     rnd.ctypes.data if rnd is not None else None, n, p.ctypes.data, nxt.ctypes.data,
                                     sh.ctypes.data, con.ctypes.data))
    return Shaded(Paths(p, p.view(np.int32)), nxt, sh, con)


def _camera_opts(sample, first_pixel, tag_stride, tag_offset):
    o = CameraOpts()
    o.first_pixel, o.sample, o.tag_stride, o.tag_offset = int(first_pixel), int(sample), int(tag_stride), int(tag_offset)
    return o


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
    _check(lib().rt_debug_camera_paths_host(C.byref(uniforms), C.byref(o), rnd.ctypes.data, n, rays.ctypes.data,
                                            p.ctypes.data))
    return rays, Paths(p, p.view(np.int32))


def glass_override():
    o = MaterialOverride()
    lib().rt_material_override_glass(C.byref(o))
    return o


class Scene:
    """Host scene (Scene.swift / AppScene.swift / Model.swift OBJ path)."""

    def __init__(self, handle=None):
        if handle is None:
            h = C.c_void_p()
            _check(lib().rt_scene_new(C.byref(h)))
            handle = h
        self._h = handle
        self.synthetic = False

    @classmethod
    def preset(cls, name, asset_dir=None):
        h = C.c_void_p()
        synth = C.c_int32(0)
        st = lib().rt_scene_preset(name.encode(), (asset_dir or ASSET_DIR_DEFAULT).encode(), C.byref(h),
                                   C.byref(synth))
        if st != 0:
            msg = lib().rt_scene_last_error(h) if h.value else lib().rt_last_error(None)
            if h.value:
                lib().rt_scene_free(h)
            raise RTError(st, (msg or b"").decode())
        s = cls(h)
        s.synthetic = bool(synth.value)
        return s

    def add_model(self, obj_path, position, rotation=(0, 0, 0), scale=1.0, material_override=None):
        """Model(name:position:rotation:scale:materialOverride:) for an OBJ file."""
        p = (C.c_float * 3)(*position)
        r = (C.c_float * 3)(*rotation)
        _check(lib().rt_scene_add_obj(self._h, obj_path.encode(), p, r, scale,
                                      C.byref(material_override) if material_override else None), scene=self._h)

    def add_usd(self, usd_path, position, rotation=(0, 0, 0), scale=1.0, material_override=None):
        """Model(name:...) for a .usdz / .usda / .usdc asset (Model.swift:87-184)."""
        p = (C.c_float * 3)(*position)
        r = (C.c_float * 3)(*rotation)
        _check(lib().rt_scene_add_usd(self._h, usd_path.encode(), p, r, scale,
                                      C.byref(material_override) if material_override else None), scene=self._h)

    def add_procedural(self, kind, position, rotation=(0, 0, 0), scale=1.0, material_override=None, mtl_path=None):
        p = (C.c_float * 3)(*position)
        r = (C.c_float * 3)(*rotation)
        _check(lib().rt_scene_add_procedural(self._h, kind.encode(), mtl_path.encode() if mtl_path else None, p, r,
                                             scale, C.byref(material_override) if material_override else None),
               scene=self._h)

    def add_texture(self, rgba8):
        """Adds an (H, W, 4) uint8 texture (row 0 = top); returns its id."""
        a = np.ascontiguousarray(rgba8, dtype=np.uint8)
        assert a.ndim == 3 and a.shape[2] == 4, a.shape
        tid = C.c_uint32(0)
        _check(lib().rt_scene_add_texture(self._h, a.ctypes.data, a.shape[1], a.shape[0], C.byref(tid)), scene=self._h)
        return tid.value

    def load_texture(self, png_path):
        """Decodes a PNG file into the scene's textures (MTKTextureLoader stand-in); returns its id."""
        tid = C.c_uint32(0)
        _check(lib().rt_scene_load_texture(self._h, png_path.encode(), C.byref(tid)), scene=self._h)
        return tid.value

    def bind_texture(self, mesh_index, submesh_index, slot, texture_id):
        """slot: 'baseColor' | 'normal' | 'roughness' | 'metallic' | 'ao' | 'emission' | 'opacity'
        (or its index).  Sets the material's textureFlags bit (and baseColor = 1 for baseColor)."""
        k = TEXTURE_SLOTS[slot] if isinstance(slot, str) else int(slot)
        _check(lib().rt_scene_bind_texture(self._h, mesh_index, submesh_index, k, texture_id), scene=self._h)

    def set_lights(self, lights):
        arr = (Light * len(lights))(*lights)
        _check(lib().rt_scene_set_lights(self._h, arr, len(lights)), scene=self._h)

    def set_light_intensity(self, intensity):
        _check(lib().rt_scene_set_light_intensity(self._h, intensity), scene=self._h)

    def desc(self):
        d = SceneDesc()
        _check(lib().rt_scene_get_desc(self._h, C.byref(d)), scene=self._h)
        return d

    @property
    def triangle_count(self):
        return int(lib().rt_scene_triangle_count(self._h))

    @property
    def light_count(self):
        return int(self.desc().light_count)

    def joint_matrices(self, mesh_index, time_seconds, capacity=256):
        out = np.zeros((capacity, 16), dtype=np.float32)
        n = C.c_uint32(0)
        _check(lib().rt_scene_joint_matrices(self._h, mesh_index, time_seconds,
                                             out.ctypes.data_as(C.POINTER(C.c_float)), capacity, C.byref(n)),
               scene=self._h)
        return out[: n.value].copy()

    def close(self):
        if self._h:
            lib().rt_scene_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_KNOBS = {
    # Renderer.swift:52-192 property -> (Uniforms field, default)
    "samplesPerPixel": ("samplesPerPixel", 2),
    "maxBounces": ("maxBounces", 2),
    "accumulationWeight": ("accumulationWeight", 0.9),
    "useMotionAdaptiveAccumulation": ("enableMotionAdaptiveAccumulation", True),
    "motionAccumulationMinWeight": ("motionAccumulationMinWeight", 0.1),
    "motionAccumulationLowThresholdPixels": ("motionAccumulationLowThresholdPixels", 0.5),
    "motionAccumulationHighThresholdPixels": ("motionAccumulationHighThresholdPixels", 4.0),
    "useMotionAdaptiveSampling": ("enableMotionAdaptiveSampling", True),
    "motionSamplingMaxExtraSamples": ("motionSamplingMaxExtraSamples", 2),
    "motionSamplingLowThresholdPixels": ("motionSamplingLowThresholdPixels", 1.0),
    "motionSamplingHighThresholdPixels": ("motionSamplingHighThresholdPixels", 6.0),
    "debugTextureMode": ("debugTextureMode", 0),
    "shadingMode": ("shadingMode", 0),
    "useTemporalDenoiser": ("enableDenoiseGBuffer", False),
}


# Legacy environment names of the rt_tuning fields (and of three rt_opts / rt_set_graphs settings),
# read by tuning_from_env for the test and bench harnesses only: the library itself reads none.
_TUNING_ENV = {"RT_CHUNK": "trace_chunk", "RT_FCHUNK": "finish_chunk", "RT_REFILL_MIN": "refill_min",
               "RT_SHADE_MIN": "shade_min", "RT_SHADE_MIN_X": "shade_min_drained", "RT_TEAM": "team",
               "RT_FINISH_FRAC": "finish_grid_pct", "RT_TRACE_FRAC": "trace_grid_pct", "RT_SHADE_BLOCKS": "shade_blocks",
               "RT_WF_HOST": "host_rounds", "RT_WF_LOG": "log", "RT_DEVICE_BVH": "device_bvh"}


def tuning_from_env(environ=None):
    """Harness convenience (bench.py, the tests' child processes): the rt_tuning fields named by the
    legacy RT_* environment variables (RT_TEAM: 0 = off, as before; RT_DEVICE_BVH=lbvh), plus
    'tail_paths' (RT_TAIL_RAYS), 'frames_in_flight' (RT_FRAMES_IN_FLIGHT) and 'graphs' (RT_GRAPH).
    The library reads no environment variable: a caller sets these with Renderer(tuning=...) /
    rt_set_tuning, rt_opts and rt_set_graphs."""
    env = os.environ if environ is None else environ
    out = {}
    for name, field in _TUNING_ENV.items():
        v = env.get(name)
        if v is None or v == "":
            continue
        if field == "team":
            out[field] = 1 if int(v) in (0, 1) else int(v)
        elif field == "device_bvh":
            out[field] = 1 if v == "lbvh" else 0
        else:
            out[field] = int(v)
    for name, key in (("RT_TAIL_RAYS", "tail_paths"), ("RT_FRAMES_IN_FLIGHT", "frames_in_flight"), ("RT_GRAPH", "graphs")):
        if env.get(name):
            out[key] = int(env[name])
    return out


def _tuning_struct(fields):
    t = Tuning()
    for k, v in fields.items():
        if not hasattr(t, k) or k == "reserved":
            raise KeyError(f"unknown rt_tuning field {k!r}")
        setattr(t, k, int(v))
    return t


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


class Renderer:
    """Renderer.swift for the hot path: owns a device context, the uniforms and the frame index.

    Setting any knob resets frameIndex to 0 (the reference's didSet { frameIndex = 0 }).
    draw() = updateUniforms + raytracingKernel dispatch + accumulation swap.
    """

    def __init__(self, scene, width, height, device=0, pipeline="wavefront", seed=1, stream=None, tail_paths=0,
                 sort_bins=0, bvh="sah", frames_in_flight=0, tuning=None):
        object.__setattr__(self, "_ctx", None)
        self.scene = scene
        self.width, self.height = int(width), int(height)
        opts = _abi.Opts()
        opts.device = device
        opts.pipeline = {"megakernel": 0, "wavefront": 1}[pipeline]
        opts.tail_paths = int(tail_paths)
        opts.sort_bins = int(sort_bins)   # 0 = default hit sort, < 0 = none
        opts.frames_in_flight = int(frames_in_flight)   # 0 = default (one per HIP hardware queue: 4, or 8 with GPU_MAX_HW_QUEUES >= 8; within a 96 GB budget, >= 2), 1 = one frame at a time
        ctx = C.c_void_p()
        _check(lib().rt_create(C.byref(opts), C.byref(ctx)))
        object.__setattr__(self, "_ctx", ctx)
        self.device = int(device)
        if stream is not None:
            _check(lib().rt_set_stream(ctx, C.c_void_p(stream)), ctx)
        if tuning:
            self.set_tuning(**tuning)
        d = scene.desc()
        self.light_count = int(d.light_count)
        _check(lib().rt_scene_upload(ctx, C.byref(d)), ctx)
        self.bvh_builder = bvh   # "sah": host binned-SAH build; "lbvh": on-device build
        _check((lib().rt_bvh_build_device if bvh == "lbvh" else lib().rt_bvh_build)(ctx), ctx)
        self.random = random_offsets(seed, self.width, self.height)
        _check(lib().rt_resize(ctx, self.width, self.height, self.random.ctypes.data_as(C.POINTER(C.c_uint32))), ctx)
        self.camera = camera_default(self.width, self.height)
        self.previousCamera = None
        self.frameIndex = 0
        self._knobs = {k: v for k, (_, v) in _KNOBS.items()}

    def __getattr__(self, name):
        knobs = self.__dict__.get("_knobs")
        if knobs is not None and name in knobs:
            return knobs[name]
        raise AttributeError(name)

    def __setattr__(self, name, value):
        if name in _KNOBS and "_knobs" in self.__dict__:
            self._knobs[name] = value
            self.__dict__["frameIndex"] = 0  # didSet { frameIndex = 0 }
            return
        object.__setattr__(self, name, value)

    # --- Renderer.updateUniforms (Renderer.swift:608-664) ---
    def uniforms(self):
        u = uniforms_default(self.width, self.height, self.light_count)
        for k, (field, _) in _KNOBS.items():
            v = self._knobs[k]
            setattr(u, field, int(v) if isinstance(v, bool) else v)
        u.camera = self.camera
        u.previousCamera = self.previousCamera if self.previousCamera is not None else self.camera
        u.frameIndex = self.frameIndex
        return u

    def draw(self, tiles=None):
        u = self.uniforms()
        ts = None
        if tiles is not None:
            ts = TileSet(tiles[0], tiles[1], tiles[2], 0)
        _check(lib().rt_render_frame(self._ctx, C.byref(u), C.byref(ts) if ts else None), self._ctx)
        self.__dict__["frameIndex"] = self.frameIndex + 1
        self.previousCamera = self.camera
        return u

    def set_tuning(self, **fields):
        """rt_set_tuning: the wavefront kernels' scheduling parameters (rt_tuning fields; omitted = default)."""
        _check(lib().rt_set_tuning(self._ctx, C.byref(_tuning_struct(fields))), self._ctx)

    def tuning(self):
        """rt_get_tuning: the parameters in effect, defaults resolved."""
        t = Tuning()
        _check(lib().rt_get_tuning(self._ctx, C.byref(t)), self._ctx)
        return {n: getattr(t, n) for n, _ in Tuning._fields_ if n != "reserved"}

    def wait(self):
        _check(lib().rt_wait(self._ctx), self._ctx)

    def set_counting(self, on):
        _check(lib().rt_set_counting(self._ctx, 1 if on else 0), self._ctx)

    def set_device_spans(self, on):
        """Device-clock launch spans in the stats (rt_set_device_spans; measurement only)."""
        _check(lib().rt_set_device_spans(self._ctx, 1 if on else 0), self._ctx)

    def set_graphs(self, on):
        """Frames captured as HIP graphs and replayed (default) or enqueued launch by launch
        (rt_set_graphs); frames enqueued eagerly always record their per-stage times."""
        _check(lib().rt_set_graphs(self._ctx, 1 if on else 0), self._ctx)

    def stats(self):
        s = Stats()
        _check(lib().rt_get_stats(self._ctx, C.byref(s)), self._ctx)
        return s

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

    def trace(self, rays, any_hit=False, out=None, stream=None):
        """rt_trace_closest / rt_trace_any: traces (n, 8) rays (make_rays) against the geometry the
        next draw() would see.

        Device path: `rays` is a contiguous float32 torch tensor on the renderer's device, read in
        place; the query is enqueued on `stream` (a HIP stream handle as in pack_tiles: 0 = HIP's
        null stream, torch's default; None = the renderer's stream) without a host wait, and the
        caller orders `rays` (and `out`: (n, 8) float32, or (n,) int32 for any_hit) before that
        stream.  Returns Hits (views of one (n, 8) tensor), or one int32 tensor of 1 / 0 for any_hit.

        Host path: `rays` is a host array; it is staged through torch, the query is waited for and
        the result comes back as numpy."""
        import torch
        dev = torch.device("cuda", self.device)
        host = not isinstance(rays, torch.Tensor)
        if host:
            r = torch.from_numpy(np.ascontiguousarray(rays, np.float32).reshape(-1, 8)).to(dev)
        else:
            r = rays
            if r.dtype != torch.float32 or r.dim() != 2 or r.shape[1] != 8 or not r.is_contiguous() or r.device != dev:
                raise ValueError(f"rays must be a contiguous float32 (n, 8) tensor on {dev}")
        n = r.shape[0]
        if out is None:
            out = torch.empty((n,), dtype=torch.int32, device=dev) if any_hit else \
                torch.empty((n, 8), dtype=torch.float32, device=dev)
        else:
            want = ((n,), torch.int32) if any_hit else ((n, 8), torch.float32)
            if tuple(out.shape) != want[0] or out.dtype != want[1] or not out.is_contiguous() or out.device != dev:
                raise ValueError(f"out must be a contiguous {want[1]} tensor of shape {want[0]} on {dev}")
        if host:
            torch.cuda.current_stream(dev).synchronize()   # the staging copy and the allocator's stream
        L = lib()
        args = (self._ctx, C.c_void_p(r.data_ptr()), n, C.c_void_p(out.data_ptr()))
        if stream is None:
            _check((L.rt_trace_any if any_hit else L.rt_trace_closest)(*args), self._ctx)
        else:
            _check((L.rt_trace_any_on if any_hit else L.rt_trace_closest_on)(*args, C.c_void_p(stream)), self._ctx)
        if host:
            self.wait()
            res = out.cpu().numpy()
            return res if any_hit else Hits(res, res.view(np.int32))
        return out if any_hit else Hits(out, out.view(torch.int32))

    def resolve(self, rays, hits, material=True, out=None, stream=None):
        """rt_resolve_hits: turns (n, 8) rays and their closest-hit records (a Hits object or its
        (n, 8) buffer) into surface and material records: what the renderer itself would shade at
        each hit, bit for bit, against the geometry the next draw() would see.

        Device path (`rays` is a torch tensor; so is the hit buffer): enqueued on `stream` (as in
        trace: 0 = HIP's null stream, None = the renderer's) without a host wait.  `out` is an
        (n, 16) float32 tensor, or a pair of it and an (n, 12) one; with material=False no material
        record is written.  Host path (`rays` is a host array): staged through torch, waited for,
        returned as numpy.  Returns a Surface."""
        import torch
        dev = torch.device("cuda", self.device)
        hb = hits.buffer if isinstance(hits, Hits) else hits
        host = not isinstance(rays, torch.Tensor)
        if host:
            r = torch.from_numpy(np.ascontiguousarray(rays, np.float32).reshape(-1, 8)).to(dev)
            if isinstance(hb, torch.Tensor):
                raise ValueError("rays on the host but hits on the device")
            hb = np.ascontiguousarray(hb)
            if hb.dtype != np.float32 or hb.ndim != 2 or hb.shape[1] != 8:
                raise ValueError("hits must be float32 (n, 8) rt_ray_hit records")
            h = torch.from_numpy(hb).to(dev)
        else:
            r, h = rays, hb
            for name, x in (("rays", r), ("hits", h)):
                if (not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.dim() != 2 or x.shape[1] != 8
                        or not x.is_contiguous() or x.device != dev):
                    raise ValueError(f"{name} must be a contiguous float32 (n, 8) tensor on {dev}")
        n = r.shape[0]
        if h.shape[0] != n:
            raise ValueError(f"{n} rays but {h.shape[0]} hit records")
        surf, mat = (out if isinstance(out, (tuple, list)) else (out, None)) if out is not None else (None, None)
        for name, x, cols in (("surfaces", surf, 16), ("materials", mat, 12)):
            if x is not None and (not isinstance(x, torch.Tensor) or tuple(x.shape) != (n, cols) or x.dtype != torch.float32
                                  or not x.is_contiguous() or x.device != dev):
                raise ValueError(f"out {name} must be a contiguous float32 ({n}, {cols}) tensor on {dev}")
        if mat is not None and not material:
            raise ValueError("a materials tensor was given with material=False")
        if surf is None:
            surf = torch.empty((n, 16), dtype=torch.float32, device=dev)
        if material and mat is None:
            mat = torch.empty((n, 12), dtype=torch.float32, device=dev)
        if host:
            torch.cuda.current_stream(dev).synchronize()   # the staging copies and the allocator's stream
        args = (self._ctx, C.c_void_p(r.data_ptr()), C.c_void_p(h.data_ptr()), n, C.c_void_p(surf.data_ptr()),
                C.c_void_p(mat.data_ptr()) if material else None)
        if stream is None:
            _check(lib().rt_resolve_hits(*args), self._ctx)
        else:
            _check(lib().rt_resolve_hits_on(*args, C.c_void_p(stream)), self._ctx)
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
              stream=None):
        """rt_shade_hits: what the renderer does between a resolved hit and the next ray.  `rays`
        are the (n, 8) rays that were traced, `surface` their Surface from resolve (with
        materials), `paths` a Paths (make_paths) or its (n, 12) buffer.  Returns a Shaded: the
        paths updated, next_rays to trace where paths.alive, shadow_rays to trace_any where
        paths.shadow, contrib to add to paths.radiance where those are not occluded.
        shading_mode, max_bounces and light_count default to the Renderer's current uniforms;
        randoms: None = the renderer's Halton numbers, or (n, 8) float32 (light, area u, area v,
        glass choice, r0, r1, 0, 0).

        Device path (`rays` is a torch tensor; so are the others): `paths` is updated IN PLACE,
        enqueued on `stream` (as in trace) without a host wait; `out` is a triple of float32
        tensors (next_rays (n, 8), shadow_rays (n, 8), contrib (n, 4)); next_rays may be `rays`.
        Host path (`rays` is a host array): staged through torch, waited for, returned as numpy;
        the given paths are not modified."""
        import torch
        dev = torch.device("cuda", self.device)
        host = not isinstance(rays, torch.Tensor)
        pb = paths.buffer if isinstance(paths, Paths) else paths
        sb, mb = surface.buffer, surface.material_buffer
        if mb is None:
            raise ValueError("shade needs the material records (resolve with material=True)")
        named = [("rays", rays, 8), ("surface", sb, 16), ("materials", mb, 12), ("paths", pb, 12)]
        if randoms is not None:
            named.append(("randoms", randoms, 8))
        if host:
            staged = []
            for name, x, cols in named:
                if isinstance(x, torch.Tensor):
                    raise ValueError(f"rays on the host but {name} on the device")
                x = np.ascontiguousarray(x)
                if x.dtype != np.float32 or x.ndim != 2 or x.shape[1] != cols:
                    raise ValueError(f"{name} must be float32 (n, {cols}) records")
                staged.append(torch.from_numpy(x).to(dev))
        else:
            staged = [x for _, x, _ in named]
            for name, x, cols in named:
                if (not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.dim() != 2 or x.shape[1] != cols
                        or not x.is_contiguous() or x.device != dev):
                    raise ValueError(f"{name} must be a contiguous float32 (n, {cols}) tensor on {dev}")
        n = staged[0].shape[0]
        for (name, _, _), x in zip(named, staged):
            if x.shape[0] != n:
                raise ValueError(f"{n} rays but {x.shape[0]} {name} records")
        r, s, m, p = staged[:4]
        rnd = staged[4] if randoms is not None else None
        if out is not None and (not isinstance(out, (tuple, list)) or len(out) != 3):
            raise ValueError("out must be (next_rays, shadow_rays, contrib)")
        outs = []
        for k, (name, cols) in enumerate((("next_rays", 8), ("shadow_rays", 8), ("contrib", 4))):
            x = out[k] if out is not None else torch.empty((n, cols), dtype=torch.float32, device=dev)
            if (not isinstance(x, torch.Tensor) or tuple(x.shape) != (n, cols) or x.dtype != torch.float32
                    or not x.is_contiguous() or x.device != dev):
                raise ValueError(f"out {name} must be a contiguous float32 ({n}, {cols}) tensor on {dev}")
            outs.append(x)
        o = _shade_opts(self.shadingMode if shading_mode is None else shading_mode,
                        self.maxBounces if max_bounces is None else max_bounces,
                        self.light_count if light_count is None else light_count)
        if host:
            torch.cuda.current_stream(dev).synchronize()   # the staging copies and the allocator's stream
        vp = C.c_void_p
        args = (self._ctx, C.byref(o), vp(r.data_ptr()), vp(s.data_ptr()), vp(m.data_ptr()),
                vp(rnd.data_ptr()) if rnd is not None else None, n, vp(p.data_ptr()), vp(outs[0].data_ptr()),
                vp(outs[1].data_ptr()), vp(outs[2].data_ptr()))
        if stream is None:
            _check(lib().rt_shade_hits(*args), self._ctx)
        else:
            _check(lib().rt_shade_hits_on(*args, vp(stream)), self._ctx)
        if host:
            self.wait()
            pn = p.cpu().numpy()
            return Shaded(Paths(pn, pn.view(np.int32)), *(x.cpu().numpy() for x in outs))
        return Shaded(paths if isinstance(paths, Paths) else Paths(p, p.view(torch.int32)), *outs)

    # --- path queries: the glue of a query integrator as library calls ---
    def _records(self, x, name, cols=None, rows=None, dtypes=None):
        """A contiguous 2-D tensor of 4-byte elements on the renderer's device (cols: an int or the
        allowed widths), or ValueError."""
        import torch
        dev = torch.device("cuda", self.device)
        dtypes = dtypes or (torch.float32,)
        cols_ok = (cols,) if isinstance(cols, int) else cols
        if (not isinstance(x, torch.Tensor) or x.dtype not in dtypes or x.dim() != 2 or not x.is_contiguous()
                or x.device != dev or (cols_ok is not None and x.shape[1] not in cols_ok)
                or (rows is not None and x.shape[0] != rows)):
            raise ValueError(f"{name} must be a contiguous {' / '.join(str(d) for d in dtypes)} "
                             f"({'n' if rows is None else rows}, {cols}) tensor on {dev}")
        return x

    def _words(self, x, name, rows=None):
        """A contiguous int32 vector on the renderer's device, or ValueError."""
        import torch
        dev = torch.device("cuda", self.device)
        if (not isinstance(x, torch.Tensor) or x.dtype != torch.int32 or x.dim() != 1 or not x.is_contiguous()
                or x.device != dev or (rows is not None and x.shape[0] != rows)):
            raise ValueError(f"{name} must be a contiguous int32 ({'n' if rows is None else rows},) tensor on {dev}")
        return x

    def _torch_stream(self, stream):
        """The torch stream of a HIP stream handle (0 = torch's default stream)."""
        import torch
        dev = torch.device("cuda", self.device)
        return torch.cuda.default_stream(dev) if not stream else torch.cuda.ExternalStream(stream, device=dev)

    def camera_paths(self, sample, first_pixel=0, n=None, uniforms=None, random_offsets=None, tag_stride=1, tag_offset=0,
                     out=None, stream=None):
        """rt_camera_paths: the renderer's primary rays and path states of sample `sample` for the n
        pixels from first_pixel on (row-major; default: the rest of the image), by the given
        uniforms (default: the Renderer's current ones: camera, size, frameIndex, samplesPerPixel).
        random_offsets: None = the renderer's own, or width * height offsets as an int32 tensor on
        the device (a host array is staged).  Each path's tag is pixel * tag_stride + tag_offset.
        `out` is a pair of float32 tensors ((n, 8) rays, (n, 12) paths).  Enqueued on `stream` (as
        in trace) without a host wait.  Returns (rays, Paths)."""
        import torch
        dev = torch.device("cuda", self.device)
        u = uniforms if uniforms is not None else self.uniforms()
        if n is None:
            n = u.width * u.height - int(first_pixel)
        if n < 0:
            raise ValueError("first_pixel is past the image")
        rnd = random_offsets
        if rnd is not None:
            if not isinstance(rnd, torch.Tensor):
                rnd = torch.from_numpy(np.ascontiguousarray(rnd, np.uint32).reshape(-1).view(np.int32)).to(dev)
                torch.cuda.current_stream(dev).synchronize()   # the staging copy
            self._words(rnd, "random_offsets", u.width * u.height)
        if out is not None and (not isinstance(out, (tuple, list)) or len(out) != 2):
            raise ValueError("out must be (rays, paths)")
        rays = self._records(out[0], "out rays", 8, n) if out is not None else torch.empty((n, 8), dtype=torch.float32, device=dev)
        pb = self._records(out[1], "out paths", 12, n) if out is not None else torch.empty((n, 12), dtype=torch.float32, device=dev)
        o = _camera_opts(sample, first_pixel, tag_stride, tag_offset)
        vp = C.c_void_p
        args = (self._ctx, C.byref(u), C.byref(o), vp(rnd.data_ptr()) if rnd is not None else None, n, vp(rays.data_ptr()),
                vp(pb.data_ptr()))
        if stream is None:
            _check(lib().rt_camera_paths(*args), self._ctx)
        else:
            _check(lib().rt_camera_paths_on(*args, vp(stream)), self._ctx)
        return rays, Paths(pb, pb.view(torch.int32))

    def compact(self, paths, mask, streams=(), index=True, out=None, stream=None):
        """rt_compact_paths: stable compaction of up to four record streams by the paths' flags:
        the records i with paths.flags[i] & mask != 0, in ascending i, what x[(flags & mask) != 0]
        gives.  `paths` is a Paths or its (n, 12) buffer; `streams` are (n, 4 * words) tensors of
        4-byte elements, words 1 .. 4 (the paths buffer itself may be one).  index: True = also
        return the selected positions, False = not, or an int32 (n,) tensor to write them to.
        out: a Compacted of an earlier call of the same shapes, or a tuple (outs, index, count) of
        tensors to write to (outs: one per stream, same shape and type; index / count may be None).
        Not in place: no output may be an input.  Enqueued on `stream` (as in trace) without a
        host wait; Compacted.n() reads the count back."""
        import torch
        dev = torch.device("cuda", self.device)
        four = (torch.float32, torch.int32)
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
        outs = []
        for k, x in enumerate(srcs):
            d = o_outs[k] if o_outs is not None else torch.empty_like(x)
            self._records(d, f"out {k}", x.shape[1], n, (x.dtype,))
            outs.append(d)
        if isinstance(index, torch.Tensor):
            idx = self._words(index, "index", n)
        elif index:
            idx = self._words(o_index, "out index", n) if o_index is not None else torch.empty((n,), dtype=torch.int32, device=dev)
        else:
            idx = None
        count = self._words(o_count, "out count", 1) if o_count is not None else torch.empty((1,), dtype=torch.int32, device=dev)
        if host is None:
            host = torch.empty((1,), dtype=torch.int32, pin_memory=True)
        arr = (CompactStream * max(len(srcs), 1))()
        for k, (x, d) in enumerate(zip(srcs, outs)):
            arr[k].src, arr[k].dst, arr[k].words = x.data_ptr(), d.data_ptr(), x.shape[1] // 4
        vp = C.c_void_p
        if n == 0:   # nothing is launched and nothing written: the count is ours to set
            with torch.cuda.stream(self._torch_stream(stream) if stream is not None else torch.cuda.current_stream(dev)):
                count.zero_()
        args = (self._ctx, vp(pb.data_ptr()), n, int(mask), arr, len(srcs), vp(idx.data_ptr()) if idx is not None else None,
                vp(count.data_ptr()))
        if stream is None:
            _check(lib().rt_compact_paths(*args), self._ctx)
        else:
            _check(lib().rt_compact_paths_on(*args, vp(stream)), self._ctx)

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

    def connect(self, paths, contrib, occluded, index=None, m=None, stream=None):
        """rt_connect_paths: paths.radiance[i] += contrib[i] for the first m shadow rays j that
        are not occluded (occluded[j] == 0), i = index[j] (or j without an index).  `paths`
        (Paths or buffer) is updated IN PLACE; contrib is (n, 4) float32, occluded and index int32
        vectors of at least m entries (m defaults to len(occluded)).  The index entries must be
        distinct, as compact() makes them.  Enqueued on `stream` without a host wait."""
        pb = self._records(paths.buffer if isinstance(paths, Paths) else paths, "paths", 12)
        n = pb.shape[0]
        con = self._records(contrib, "contrib", 4, n)
        occ = self._words(occluded, "occluded")
        idx = self._words(index, "index") if index is not None else None
        m = occ.shape[0] if m is None else int(m)
        if m < 0 or m > occ.shape[0] or (idx is not None and m > idx.shape[0]):
            raise ValueError(f"m = {m} is more than occluded / index hold")
        vp = C.c_void_p
        args = (self._ctx, vp(pb.data_ptr()), n, vp(con.data_ptr()), vp(idx.data_ptr()) if idx is not None else None,
                vp(occ.data_ptr()), m)
        if stream is None:
            _check(lib().rt_connect_paths(*args), self._ctx)
        else:
            _check(lib().rt_connect_paths_on(*args, vp(stream)), self._ctx)

    def retire(self, paths, samples, stream=None):
        """rt_retire_paths: samples[tag] = (radiance, 1) for every path that is not ALIVE and whose
        tag is below len(samples); `samples` is a (tags, 4) float32 tensor.  Enqueued on `stream`
        without a host wait."""
        pb = self._records(paths.buffer if isinstance(paths, Paths) else paths, "paths", 12)
        sm = self._records(samples, "samples", 4)
        vp = C.c_void_p
        args = (self._ctx, vp(pb.data_ptr()), pb.shape[0], vp(sm.data_ptr()), sm.shape[0])
        if stream is None:
            _check(lib().rt_retire_paths(*args), self._ctx)
        else:
            _check(lib().rt_retire_paths_on(*args, vp(stream)), self._ctx)

    def average(self, samples, spp, out=None, stream=None):
        """rt_average_samples: (pixels * spp, 4) float32 samples, a pixel's spp samples side by
        side, into (pixels, 4): their sum in sample order / spp, alpha 1, as the renderer resolves
        frame 0.  Enqueued on `stream` without a host wait.  Returns the (pixels, 4) tensor."""
        import torch
        sm = self._records(samples, "samples", 4)
        spp = int(spp)
        if spp < 1 or sm.shape[0] % spp:
            raise ValueError(f"{sm.shape[0]} samples are not a multiple of spp = {spp}")
        pixels = sm.shape[0] // spp
        if out is None:
            out = torch.empty((pixels, 4), dtype=torch.float32, device=sm.device)
        self._records(out, "out", 4, pixels)
        vp = C.c_void_p
        args = (self._ctx, vp(sm.data_ptr()), pixels, spp, vp(out.data_ptr()))
        if stream is None:
            _check(lib().rt_average_samples(*args), self._ctx)
        else:
            _check(lib().rt_average_samples_on(*args, vp(stream)), self._ctx)
        return out

    def _path_buffers(self, cap, tags):
        """path_trace's working set, allocated once per size: two sets of rays and paths to
        ping-pong between, one of everything else."""
        import torch
        have = self.__dict__.get("_pt_buffers")
        if have is not None and have["cap"] == cap and have["tags"] == tags:
            return have
        dev = torch.device("cuda", self.device)
        f = lambda cols, rows=cap: torch.empty((rows, cols), dtype=torch.float32, device=dev)
        w = lambda rows=cap: torch.empty((rows,), dtype=torch.int32, device=dev)
        pin = lambda: torch.empty((1,), dtype=torch.int32, pin_memory=True)
        b = dict(cap=cap, tags=tags, rays=[f(8), f(8)], paths=[f(12), f(12)], hits=f(8), surf=f(16), mat=f(12), nxt=f(8),
                 shadow=f(8), contrib=f(4), shadow_c=f(8), sh_index=w(), occluded=w(), samples=f(4, tags),
                 counts=[w(1), w(1)], pinned=[pin(), pin()])
        self._pt_buffers = b
        return b

    def path_trace(self, spp=None, max_bounces=None, shading_mode=None, stream=0, batch_samples=True):
        """Frame 0 of the current uniforms from queries only: camera_paths, then per round
        trace -> resolve -> shade -> compact(SHADOW: shadow rays + index) -> trace(any_hit) ->
        connect -> retire -> compact(ALIVE: next rays + paths) until no path is left, then
        average.  Bit-identical to draw() + radiance() of frame 0 in all four channels.  The host's
        part per round is reading the two compactions' counts.  batch_samples: all samples of the
        image in one array (tag = pixel * spp + s), else one sample at a time.  Runs on `stream`
        (as in trace; default 0 = torch's default stream); the working buffers are allocated once
        per size and kept.  Returns the (H, W, 4) float32 tensor, valid on that stream; the ray
        totals are kept in `last_path_trace` (closest_rays, shadow_rays, paths, rounds)."""
        import torch
        dev = torch.device("cuda", self.device)
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
        A, SH = Paths.ALIVE, Paths.SHADOW
        q = dict(stream=stream)
        totals = dict(closest_rays=0, shadow_rays=0, paths=pixels * spp, rounds=0)
        for group in ([range(spp)] if batch_samples else [[s] for s in range(spp)]):
            cur = 0
            for s in group:
                k = s * pixels if batch_samples else 0
                self.camera_paths(s, uniforms=u, tag_stride=spp, tag_offset=s,
                                  out=(B["rays"][cur][k:k + pixels], B["paths"][cur][k:k + pixels]), **q)
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
        _check(lib().rt_get_query_stats(self._ctx, C.byref(s)), self._ctx)
        return s

    def radiance(self):
        out = np.empty((self.height, self.width, 4), dtype=np.float32)
        _check(lib().rt_read_radiance(self._ctx, out.ctypes.data_as(C.POINTER(C.c_float))), self._ctx)
        return out

    def radiance_half(self):
        """rt_read_radiance_half: the radiance as RGBA16F (the reference's accumulation format,
        Renderer.swift:685), rounded to nearest even on the device; (H, W, 4) float16."""
        out = np.empty((self.height, self.width, 4), dtype=np.float16)
        _check(lib().rt_read_radiance_half(self._ctx, out.ctypes.data_as(C.POINTER(C.c_uint16))), self._ctx)
        return out

    def aux(self, gbuffer=False):
        depth = np.empty((self.height, self.width), dtype=np.float32)
        motion = np.empty((self.height, self.width, 2), dtype=np.float32)
        gb = np.empty((4, self.height, self.width, 4), dtype=np.float32) if gbuffer else None
        FP = C.POINTER(C.c_float)
        _check(lib().rt_read_aux(self._ctx, depth.ctypes.data_as(FP), motion.ctypes.data_as(FP),
                                 gb.ctypes.data_as(FP) if gb is not None else None), self._ctx)
        return depth, motion, gb

    def set_instance_transforms(self, mats):
        """mats: (n, 4, 3) packed column-major object->world (updateInstanceDescriptors)."""
        arr = np.ascontiguousarray(mats, dtype=np.float32).reshape(-1, 12)
        _check(lib().rt_set_instance_transforms(self._ctx, arr.ctypes.data_as(C.POINTER(PackedFloat4x3)),
                                                arr.shape[0]), self._ctx)

    def skin(self, mesh_index, joints):
        j = np.ascontiguousarray(joints, dtype=np.float32)
        _check(lib().rt_skin(self._ctx, mesh_index, j.ctypes.data_as(C.POINTER(C.c_float)), j.shape[0]), self._ctx)

    def refit(self):
        _check(lib().rt_bvh_refit(self._ctx), self._ctx)

    def rebuild(self, device=None):
        """Full BVH rebuild from the current geometry (Renderer.swift:1252-1277); on the GPU when
        device is True (default: the builder this renderer was created with)."""
        dev = (self.bvh_builder == "lbvh") if device is None else device
        _check((lib().rt_bvh_build_device if dev else lib().rt_bvh_build)(self._ctx), self._ctx)

    def present(self, width=None, height=None, scaler="none", srgb=True, denoise_passes=0):
        """Display image of the newest frame (FramePresenter + Shaders.metal): resampled to
        width x height ('none' = nearest, 'spatial' = bilinear, 'temporal' = reprojected history
        through the motion vectors, 'denoised' = G-buffer-guided a-trous filter then 'temporal';
        needs useTemporalDenoiser), tone-mapped c / (1 + c), 8-bit sRGB (or linear) RGBA rows
        top-down."""
        o = _abi.PresentOpts()
        o.out_width = int(width or 0)
        o.out_height = int(height or 0)
        o.scaler = _abi.SCALERS[scaler]
        o.encode = 0 if srgb else 1
        o.denoise_passes = int(denoise_passes)
        out = np.empty((height or self.height, width or self.width, 4), dtype=np.uint8)
        _check(lib().rt_present(self._ctx, C.byref(o), out.ctypes.data), self._ctx)
        return out

    def resize(self, width, height, seed=1):
        """mtkView(_:drawableSizeWillChange:) (Renderer.swift:1505-1511): new targets and random
        offsets, frameIndex = 0.  Frames in flight finish first."""
        self.width, self.height = int(width), int(height)
        self.random = random_offsets(seed, self.width, self.height)
        _check(lib().rt_resize(self._ctx, self.width, self.height, self.random.ctypes.data_as(C.POINTER(C.c_uint32))),
               self._ctx)
        self.camera = camera_default(self.width, self.height)
        self.previousCamera = None
        self.frameIndex = 0

    def upload(self, desc):
        """Re-uploads a scene description (rt_scene_upload) and rebuilds the BVH."""
        _check(lib().rt_scene_upload(self._ctx, C.byref(desc)), self._ctx)
        self.rebuild()

    def tile_count(self, tile_size, rank, nranks):
        ts = TileSet(tile_size, rank, nranks, 0)
        return int(lib().rt_tile_count(self.width, self.height, C.byref(ts)))

    def pack_tiles(self, tile_size, rank, nranks, device_ptr, stream=None):
        """Packs this rank's tiles of the newest frame (after it, on `stream`: a HIP stream handle, 0 =
        HIP's null stream, i.e. torch's default stream; None = the renderer's stream); no host wait."""
        ts = TileSet(tile_size, rank, nranks, 0)
        if stream is None:
            _check(lib().rt_pack_tiles(self._ctx, C.byref(ts), C.c_void_p(device_ptr)), self._ctx)
        else:
            _check(lib().rt_pack_tiles_on(self._ctx, C.byref(ts), C.c_void_p(device_ptr), C.c_void_p(stream)),
                   self._ctx)

    def unpack_tiles(self, tile_size, rank, nranks, device_ptr, stream=None):
        ts = TileSet(tile_size, rank, nranks, 0)
        if stream is None:
            _check(lib().rt_unpack_tiles(self._ctx, C.byref(ts), C.c_void_p(device_ptr)), self._ctx)
        else:
            _check(lib().rt_unpack_tiles_on(self._ctx, C.byref(ts), C.c_void_p(device_ptr), C.c_void_p(stream)),
                   self._ctx)

    def set_stream(self, stream_handle):
        _check(lib().rt_set_stream(self._ctx, C.c_void_p(stream_handle) if stream_handle else None), self._ctx)

    def close(self):
        ctx = self.__dict__.get("_ctx")
        if ctx:
            lib().rt_destroy(ctx)
            object.__setattr__(self, "_ctx", None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
