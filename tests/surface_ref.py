"""Shared by tests/test_surface_host.py and tests/test_gpu_surface.py (no tests here): the camera
rays of a frame restated in float32 numpy, and the surface / material records of a batch of hits
restated from the scene descriptor.  Every expression keeps the operand order of csrc/rt_surface.h
and csrc/rt_math.h (numpy's float32 + - * / sqrt are the IEEE operations, nothing is contracted),
so the results are compared bitwise."""
import ctypes as C

import numpy as np

F = np.float32
MISS = 0xFFFFFFFF
HAS_UV, BACKFACE, NORMAL_MAPPED, TRANSMISSIVE = 1, 2, 4, 8
TEX_BASE, TEX_NORMAL, TEX_ROUGH, TEX_METAL, TEX_AO, TEX_EMIS, TEX_OPAC = (1 << k for k in range(7))
INF_BITS = 0x7F800000
# a miss: surface (0, 0, 0, inf), zeros, zeros, (MISS, MISS, MISS, 0); material all zero
MISS_SURFACE = np.array([0, 0, 0, INF_BITS] + [0] * 8 + [MISS, MISS, MISS, 0], np.uint32)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _normalize(a):
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = F(1) / np.sqrt(_dot(a, a))
        return a * inv[:, None]


def _xform0(M, p):
    """rt::xform with w = 0: ((c0 * x + c1 * y) + c2 * z) + c3 * 0, M (n, 12) column-major."""
    return ((M[:, 0:3] * p[:, 0:1] + M[:, 3:6] * p[:, 1:2]) + M[:, 6:9] * p[:, 2:3]) + M[:, 9:12] * F(0)


def _clamp01(x):
    return np.minimum(np.maximum(x, F(0)), F(1))


def _v3(a):
    return np.array([a.x, a.y, a.z], F)


def camera_rays(rt, orc, W, H, seed, camera=None):
    """Sample 0's primary rays of frame 0, pixel by pixel in row-major order, as primary_ray
    (csrc/rt_shade.h) forms them; returns (origins, directions), float32 (W * H, 3)."""
    rnd = rt.random_offsets(seed, W, H)
    cam = camera if camera is not None else rt.camera_default(W, H)
    rx = np.array([orc.halton(int(o), 0) for o in rnd], F)
    ry = np.array([orc.halton(int(o), 1) for o in rnd], F)
    px = np.tile(np.arange(W, dtype=F), H)
    py = np.repeat(np.arange(H, dtype=F), W)
    uvx = (px + rx) / F(W)
    uvy = (py + ry) / F(H)
    uvx = uvx * F(2) - F(1)
    uvy = uvy * F(2) - F(1)
    d = (uvx[:, None] * _v3(cam.right) + uvy[:, None] * _v3(cam.up)) + _v3(cam.forward)
    d = _normalize(d)
    o = np.broadcast_to(_v3(cam.position), d.shape).copy()
    return o, np.ascontiguousarray(d, F)


def _floats(ptr, n, k):
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_float)), shape=(n, k))


class SceneArrays:
    """A scene descriptor flattened the way rt_scene_upload flattens it: vertex streams with every
    mesh's vertices after the previous one's, per scene-wide triangle its three vertex ids, mesh and
    submesh, and per triangle the material fields of its submesh."""

    def __init__(self, desc):
        pos, nrm, uv, tri, mesh, sub = [], [], [], [], [], []
        mats = []
        self.max_sub = max(desc.meshes[m].submesh_count for m in range(desc.mesh_count))
        vbase = 0
        for m in range(desc.mesh_count):
            md = desc.meshes[m]
            n = md.vertex_count
            pos.append(_floats(md.positions, n, 4)[:, :3].copy())
            nrm.append(_floats(md.normals, n, 4)[:, :3].copy())
            uv.append(_floats(md.uvs, n, 2).copy() if md.uvs else np.zeros((n, 2), F))
            for s in range(md.submesh_count):
                sm = md.submeshes[s]
                k = sm.index_count // 3
                if k:
                    idx = np.ctypeslib.as_array(sm.indices, shape=(sm.index_count,)).reshape(k, 3).astype(np.int64)
                    tri.append(idx + vbase)
                mesh += [m] * k
                sub += [s] * k
                mt = sm.material
                mats += [(_v3(mt.baseColor), _v3(mt.emission), F(mt.refractionIndex), F(mt.opacity), int(mt.textureFlags),
                          list(sm.textures))] * k
            vbase += n
        self.pos, self.nrm, self.uv = np.concatenate(pos), np.concatenate(nrm), np.concatenate(uv)
        self.tri = np.concatenate(tri)
        self.mesh, self.sub = np.array(mesh, np.int64), np.array(sub, np.int64)
        self.inst = np.stack([np.frombuffer(bytes(desc.meshes[m].transform), F) for m in range(desc.mesh_count)])
        self.base = np.stack([x[0] for x in mats])
        self.emis = np.stack([x[1] for x in mats])
        self.ior = np.array([x[2] for x in mats], F)
        self.opac = np.array([x[3] for x in mats], F)
        self.tflags = np.array([x[4] for x in mats], np.uint32)
        self.tex = np.array([x[5] for x in mats], np.int64)
        self.ntris = len(self.tri)


def restate(A, osc, o, d, t, ids, u, v):
    """The records of the hits (o, d: (n, 3) rays; t, u, v and triangle ids `ids`, hits only, no
    miss among them) restated from SceneArrays A; map samples through the oracle's sampler
    (osc.tex_sample).  Returns a dict of arrays; `shading_normal` holds the plain normal (compare it
    where NORMAL_MAPPED is clear)."""
    ids = ids.astype(np.int64)
    o, d, t, u, v = (np.ascontiguousarray(x, F) for x in (o, d, t, u, v))
    tri, M = A.tri[ids], A.inst[A.mesh[ids]]
    w = (F(1) - u) - v
    i0, i1, i2 = tri[:, 0], tri[:, 1], tri[:, 2]
    pos = o + d * t[:, None]
    objN = (u[:, None] * A.nrm[i1] + v[:, None] * A.nrm[i2]) + w[:, None] * A.nrm[i0]
    Ng = _normalize(_xform0(M, objN))
    degenerate = _dot(objN, objN) < F(float.fromhex("0x1.79ca1p-67"))
    Ng[degenerate] = -d[degenerate]
    raw = A.tflags[ids]
    tfl = raw & ~np.uint32(TEX_AO)
    textured = tfl != 0
    a, b, c = A.uv[i1], A.uv[i2], A.uv[i0]
    tcx = (u * a[:, 0] + v * b[:, 0]) + w * c[:, 0]
    tcy = (u * a[:, 1] + v * b[:, 1]) + w * c[:, 1]
    tcy = F(1) - tcy
    uv = np.where(textured[:, None], np.stack([tcx, tcy], axis=1), F(0)).astype(F)

    def sample(k, slot, srgb):
        return osc.tex_sample(int(A.tex[ids[k], slot]), float(uv[k, 0]), float(uv[k, 1]), srgb=srgb)

    base, emis = A.base[ids].copy(), A.emis[ids].copy()
    opac = _clamp01(A.opac[ids])
    rough, metal = np.ones(len(ids), F), np.zeros(len(ids), F)
    for k in np.flatnonzero(textured):
        if tfl[k] & TEX_BASE:
            base[k] = base[k] * sample(k, 0, True)[:3]
        if tfl[k] & TEX_ROUGH:
            rough[k] = sample(k, 2, False)[0]
        if tfl[k] & TEX_METAL:
            metal[k] = sample(k, 3, False)[0]
        if tfl[k] & TEX_OPAC:
            opac[k] = opac[k] * sample(k, 6, False)[0]
        if tfl[k] & TEX_EMIS:
            emis[k] = sample(k, 5, True)[:3]
    opac = _clamp01(opac)
    ior = np.maximum(A.ior[ids], F(1))
    # computeTangentBasis' validity (csrc/rt_surface.h tangent_basis), for RT_SURFACE_NORMAL_MAPPED
    p0, p1, p2 = A.pos[i1], A.pos[i2], A.pos[i0]
    e1, e2 = p1 - p0, p2 - p0
    d1x, d1y, d2x, d2y = b[:, 0] - a[:, 0], b[:, 1] - a[:, 1], c[:, 0] - a[:, 0], c[:, 1] - a[:, 1]
    denom = d1x * d2y - d1y * d2x
    with np.errstate(divide="ignore", invalid="ignore"):
        r = F(1) / denom
        tangent = (e1 * d2y[:, None] - e2 * d1y[:, None]) * r[:, None]
        bitangent = (e2 * d1x[:, None] - e1 * d2x[:, None]) * r[:, None]
        basis = (~(np.abs(denom) < F(1e-8)) & (np.sqrt(_dot(tangent, tangent)) > F(1e-8))
                 & (np.sqrt(_dot(bitangent, bitangent)) > F(1e-8)))
    flags = np.zeros(len(ids), np.uint32)
    flags[textured] |= HAS_UV
    flags[_dot(d, Ng) > F(0)] |= BACKFACE
    flags[((tfl & TEX_NORMAL) != 0) & basis] |= NORMAL_MAPPED
    flags[(opac < F(0.999)) | (ior > F(1.01))] |= TRANSMISSIVE
    return dict(position=pos, t=t, normal=Ng, uv=uv, shading_normal=Ng, triangle=ids.astype(np.int32),
                mesh=A.mesh[ids].astype(np.int32), submesh=A.sub[ids].astype(np.int32), flags=flags.view(np.int32),
                base_color=base, opacity=opac, emission=emis, ior=ior, roughness=rough, metallic=metal,
                texture_flags=raw.view(np.int32), slot=(A.mesh[ids] * A.max_sub + A.sub[ids]).astype(np.int32))


FLOAT_FIELDS = ("position", "t", "normal", "uv", "shading_normal", "base_color", "opacity", "emission", "ior",
                "roughness", "metallic")
INT_FIELDS = ("triangle", "mesh", "submesh", "flags", "texture_flags", "slot")


def hit_records(ref):
    """(n, 8) float32 rt_ray_hit records from a debug_trace_host result `ref` (t, id, u, v), with
    mesh / submesh / primitive zero on hits (with_owners fills the first two in): what resolve
    reads of a record is t, u, v and the triangle; mesh and submesh are copied through."""
    n = len(ref["id"])
    h = np.zeros((n, 8), F)
    hi = h.view(np.uint32)
    h[:, 0], h[:, 1], h[:, 2] = ref["t"], ref["u"], ref["v"]
    hi[:, 3] = ref["id"]
    miss = ref["id"] == MISS
    hi[miss, 4:7] = MISS
    return h


def with_owners(h, A):
    """Fills mesh, submesh (and a zero primitive) of the hit rows of `h` from SceneArrays."""
    hi = h.view(np.uint32)
    hit = hi[:, 3] != MISS
    ids = hi[hit, 3].astype(np.int64)
    hi[hit, 4] = A.mesh[ids]
    hi[hit, 5] = A.sub[ids]
    return h
