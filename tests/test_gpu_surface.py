"""Surface queries on the device (Renderer.resolve -> rt_resolve_hits, rq_resolve in
csrc/rt_query.hip): rays and their hit records resolved into surface and material records.

The records must equal the host hook's (rt_debug_resolve_host: the same surface_eval compiled for
the host) and, through the G-buffer, what the frame kernels themselves shade.  Every comparison is
bitwise.  Scenes, rays and host references are those of tests/test_surface_host.py."""
import ctypes as C

import numpy as np
import pytest

import surface_ref as sr
from helpers import textured_scene
from test_gpu_query import _DescScene, _desc_with, _device_rays
from test_surface_host import surface_case

pytestmark = pytest.mark.gpu

MISS = sr.MISS
SCENES = [("c1", 3000), ("textured_scene", 2000), ("c3g", 600), ("c1+train", 2000)]


def _np(x):
    return None if x is None else x.cpu().numpy()


def _resolve_np(R, rays, hits, **kw):
    """trace -> resolve results as numpy buffers (surface (n, 16), material (n, 12) or None)."""
    import torch
    S = R.resolve(rays, hits, **kw)
    R.wait()
    torch.cuda.synchronize()
    return _np(S.buffer), _np(S.material_buffer)


def _assert_buffers(got, want, what=""):
    for g, w, name in zip(got, (want.buffer, want.material_buffer), ("surface", "material")):
        assert g.shape == w.shape and np.array_equal(sr.bits(g), sr.bits(w)), (what, name)


# ---- 6. device against the host hook -------------------------------------------------------------------
@pytest.mark.parametrize("bvh", ["sah", "lbvh"])
@pytest.mark.parametrize("preset,n", SCENES)
def test_device_resolve_equals_host(rt, orc, assets, preset, n, bvh):
    c = surface_case(rt, orc, assets, preset, n)
    R = rt.Renderer(c["scene"], 16, 16, bvh=bvh)
    rays = _device_rays(rt, c["o"], c["d"])
    h = R.trace(rays)
    R.wait()
    assert np.array_equal(sr.bits(_np(h.buffer)[:, :6]), sr.bits(c["hits"][:, :6]))   # the hits the host reference resolved
    before = R.query_stats()
    _assert_buffers(_resolve_np(R, rays, h), c["host"], preset)
    miss = c["ref"]["id"] == MISS
    assert 0 < miss.sum() < len(miss)
    # the surface record does not depend on whether materials are asked for
    surf, mat = _resolve_np(R, rays, h.buffer, material=False)
    assert mat is None and np.array_equal(sr.bits(surf), sr.bits(c["host"].buffer))
    # a resolve is not a query of rt_query_stats
    after = R.query_stats()
    assert after.queries_total == before.queries_total == 1 and after.total_rays == before.total_rays == n + 4
    R.close()


@pytest.mark.parametrize("n", [1, 63, 65])
def test_device_resolve_partial_waves(rt, orc, assets, n):
    """1, 63 and 65 records (3004: test_device_resolve_equals_host): a single lane, a partial wave
    and one record past a wave, of the textured scene (both template variants take the sampler)."""
    c = surface_case(rt, orc, assets, "textured_scene", 2000)
    R = rt.Renderer(c["scene"], 16, 16)
    rays = _device_rays(rt, c["o"][:n], c["d"][:n])
    surf, mat = _resolve_np(R, rays, R.trace(rays))
    assert np.array_equal(sr.bits(surf), sr.bits(c["host"].buffer[:n]))
    assert np.array_equal(sr.bits(mat), sr.bits(c["host"].material_buffer[:n]))
    R.close()


# ---- 7. device against the renderer's own G-buffer -------------------------------------------------------
@pytest.mark.parametrize("pipeline", ["megakernel", "wavefront"])
def test_resolve_equals_renderer_gbuffer(rt, orc, assets, pipeline):
    """Sample 0's primary rays of frame 0, traced and resolved as queries, against the G-buffer of
    the frame the same Renderer drew; and that frame against one drawn without the queries."""
    W, H, seed = 96, 64, 21
    sc = textured_scene(rt, assets)
    o, d = sr.camera_rays(rt, orc, W, H, seed)
    rays = _device_rays(rt, o, d)

    def run(with_queries):
        R = rt.Renderer(sc, W, H, seed=seed, pipeline=pipeline)
        R.samplesPerPixel = 1
        R.maxBounces = 1
        R.useTemporalDenoiser = True
        S = []
        if with_queries:
            S.append(R.resolve(rays, R.trace(rays)))
        R.draw()
        if with_queries:
            S.append(R.resolve(rays, R.trace(rays)))
        R.wait()
        out = (R.radiance(), *R.aux(gbuffer=True))
        recs = [(_np(s.buffer), _np(s.material_buffer)) for s in S]
        R.close()
        return out, recs

    frame0, _ = run(False)
    frame1, recs = run(True)
    for a, b in zip(frame0, frame1):
        assert np.array_equal(sr.bits(a), sr.bits(b))
    gb = frame1[3].reshape(4, W * H, 4)
    F = np.float32
    for surf, mat in recs:
        S = rt.Surface(surf, surf.view(np.int32), mat, mat.view(np.int32))
        hit = S.triangle != -1
        mapped = (S.flags & S.NORMAL_MAPPED) != 0
        assert hit.sum() > 0 and mapped.sum() > 0 and (hit & ~mapped).sum() > 0
        metal = S.metallic[:, None]
        want = [S.base_color * (F(1) - metal), F(0.04) + (S.base_color - F(0.04)) * metal,
                S.shading_normal * F(0.5) + F(0.5), np.minimum(np.maximum(S.roughness, F(0)), F(1))[:, None]]
        for plane, (w, cols) in enumerate(zip(want, (3, 3, 3, 1))):
            assert np.array_equal(sr.bits(w[hit]), sr.bits(gb[plane][hit, :cols])), (pipeline, plane)


# ---- 8. dynamic geometry ---------------------------------------------------------------------------------
def test_resolve_then_rotate_then_resolve(rt, orc, assets):
    """tests/test_gpu_query.py::test_query_then_update_then_query with a rotation: a resolve
    enqueued before the update carries the old matrix's normals, one after it the new matrix's."""
    import torch
    c = surface_case(rt, orc, assets, "c2", 1500)
    sc, desc = c["scene"], c["scene"].desc()
    R = rt.Renderer(sc, 16, 16)
    rays = _device_rays(rt, c["o"], c["d"])
    h0 = R.trace(rays)
    s0 = R.resolve(rays, h0)   # not waited for
    mats = np.stack([np.frombuffer(bytes(desc.meshes[k].transform), np.float32).reshape(4, 3).copy()
                     for k in range(desc.mesh_count)])
    a = 0.2   # about x: it tilts the normals of a floor too
    rot = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    mats[0, :3] = (rot @ mats[0, :3].astype(np.float64).T).T.astype(np.float32)   # rows are the matrix's columns
    R.set_instance_transforms(mats)
    R.refit()
    h1 = R.trace(rays)
    s1 = R.resolve(rays, h1)
    R.wait()
    torch.cuda.synchronize()
    _assert_buffers((_np(s0.buffer), _np(s0.material_buffer)), c["host"], "before the update")
    moved = _DescScene(_desc_with(rt, desc, 0, transform=mats[0]))
    want1 = rt.debug_resolve_host(moved, c["rays"], _np(h1.buffer))
    _assert_buffers((_np(s1.buffer), _np(s1.material_buffer)), want1, "after the update")
    # the rotation shows: the second batch's hits on mesh 0 carry other normals than the same hit
    # records resolved through the old matrix, and every other mesh's are unchanged by it
    old = rt.debug_resolve_host(sc, c["rays"], _np(h1.buffer))
    on0 = want1.mesh == 0
    assert on0.any() and not np.array_equal(sr.bits(want1.normal[on0]), sr.bits(old.normal[on0]))
    assert np.array_equal(sr.bits(want1.normal[~on0]), sr.bits(old.normal[~on0]))
    assert not np.array_equal(_np(h0.buffer), _np(h1.buffer))   # and it changes what some rays hit
    R.close()


def test_resolve_after_skinning(rt, orc, assets):
    """c5 after R.skin: 512 camera rays (every 12th of the 96 x 64 frame's); the records equal the
    host hook's over the oracle-skinned mesh, and the normals the numpy restatement over
    orc.skin's normals."""
    from test_gpu_dynamic import _f4, _skinned_mesh
    sc = rt.Scene.preset("c5", assets)
    desc = sc.desc()
    m = _skinned_mesh(desc)
    md = desc.meshes[m]
    nv = md.vertex_count
    rest_p, rest_n = _f4(md.positions, nv).copy(), _f4(md.normals, nv).copy()
    ji = np.ctypeslib.as_array(md.joint_indices, shape=(nv, 4)).copy()
    jw = np.ctypeslib.as_array(md.joint_weights, shape=(nv, 4)).copy()
    J = sc.joint_matrices(m, 0.35)
    o, d = sr.camera_rays(rt, orc, 96, 64, 21)
    o, d = o[::12], d[::12]
    assert len(o) == 512
    R = rt.Renderer(sc, 16, 16)
    R.skin(m, J)
    R.refit()
    rays = _device_rays(rt, o, d)
    h = R.trace(rays)
    surf, mat = _resolve_np(R, rays, h)
    hits = _np(h.buffer)
    sp, sn = orc.skin(rest_p, rest_n, ji, jw, J)
    skinned = _desc_with(rt, desc, m, positions=sp, normals=sn)
    want = rt.debug_resolve_host(_DescScene(skinned), rt.Renderer.make_rays(o, d), hits)
    _assert_buffers((surf, mat), want, "skinned")
    hi = hits.view(np.uint32)
    hit = hi[:, 3] != MISS
    on_skinned = hit & (hi[:, 4] == m)
    assert on_skinned.sum() > 0 and (hit & ~on_skinned).sum() > 0
    ref = sr.restate(sr.SceneArrays(skinned), None, o[hit], d[hit], hits[hit, 0], hi[hit, 3], hits[hit, 1], hits[hit, 2])
    assert np.array_equal(sr.bits(surf[hit, 4:7]), sr.bits(ref["normal"]))
    # the skinning moved the normals: the rest pose gives other ones on the skinned mesh
    rest = rt.debug_resolve_host(sc, rt.Renderer.make_rays(o, d), hits)
    assert not np.array_equal(rest.normal[on_skinned], surf[on_skinned, 4:7])
    R.close()


# ---- 9. streams, output and errors -------------------------------------------------------------------------
def test_resolve_two_streams_back_to_back(rt, orc, assets):
    import torch
    c = surface_case(rt, orc, assets, "textured_scene", 2000)
    R = rt.Renderer(c["scene"], 16, 16)
    ra = _device_rays(rt, c["o"][:1500], c["d"][:1500])
    rb = _device_rays(rt, c["o"][500:], c["d"][500:])
    ha = torch.from_numpy(c["hits"][:1500]).to("cuda:0")
    hb = torch.from_numpy(c["hits"][500:]).to("cuda:0")
    outs = [(torch.empty((r.shape[0], 16), dtype=torch.float32, device="cuda:0"),
             torch.empty((r.shape[0], 12), dtype=torch.float32, device="cuda:0")) for r in (ra, rb, ra, rb)]
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    Ss = [R.resolve(ra, ha, out=outs[0], stream=s1.cuda_stream), R.resolve(rb, hb, out=outs[1], stream=s2.cuda_stream),
          R.resolve(ra, ha, out=outs[2], stream=s2.cuda_stream), R.resolve(rb, hb, out=outs[3], stream=0),
          R.resolve(ra, ha), R.resolve(rb, hb, stream=s1.cuda_stream)]   # more resolves in flight than slots
    s1.synchronize()
    s2.synchronize()
    torch.cuda.synchronize()
    R.wait()
    for k, S in enumerate(Ss):
        lo, hi = (0, 1500) if k % 2 == 0 else (500, 2004)
        assert np.array_equal(sr.bits(_np(S.buffer)), sr.bits(c["host"].buffer[lo:hi])), k
        assert np.array_equal(sr.bits(_np(S.material_buffer)), sr.bits(c["host"].material_buffer[lo:hi])), k
    assert Ss[0].buffer.data_ptr() == outs[0][0].data_ptr() and Ss[3].material_buffer.data_ptr() == outs[3][1].data_ptr()
    assert R.query_stats().queries_total == 0
    R.close()


def test_resolve_without_materials_leaves_them_untouched(rt, orc, assets):
    import torch
    c = surface_case(rt, orc, assets, "textured_scene", 2000)
    L, vp = rt.lib(), C.c_void_p
    R = rt.Renderer(c["scene"], 16, 16)
    rays = _device_rays(rt, c["o"], c["d"])
    hits = torch.from_numpy(c["hits"]).to("cuda:0")
    n = rays.shape[0]
    surf = torch.empty((n, 16), dtype=torch.float32, device="cuda:0")
    poison = torch.full((n, 12), -123.25, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    S = R.resolve(rays, hits, material=False, out=surf)
    R.wait()
    assert S.material_buffer is None and not hasattr(S, "base_color")
    assert np.array_equal(sr.bits(_np(surf)), sr.bits(c["host"].buffer))
    assert torch.all(poison == -123.25).item()
    # ... and the C entry point with a NULL materials pointer next to a live tensor
    assert L.rt_resolve_hits(R._ctx, vp(rays.data_ptr()), vp(hits.data_ptr()), n, vp(surf.data_ptr()), None) == 0
    R.wait()
    assert torch.all(poison == -123.25).item()
    with pytest.raises(ValueError):
        R.resolve(rays, hits, material=False, out=(surf, poison))
    R.close()


def test_resolve_errors(rt, orc, assets):
    import torch
    A, L = rt._abi, rt.lib()
    c = surface_case(rt, orc, assets, "c1", 3000)
    sc = c["scene"]
    rays = _device_rays(rt, c["o"][:8], c["d"][:8])
    hits = torch.from_numpy(c["hits"][:8]).to("cuda:0")
    surf = torch.empty((8, 16), dtype=torch.float32, device="cuda:0")
    mat = torch.empty((8, 12), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    vp = C.c_void_p
    r, h, s, m = (x.data_ptr() for x in (rays, hits, surf, mat))
    ctx = vp()
    assert L.rt_create(C.byref(A.Opts()), C.byref(ctx)) == A.RT_OK
    d = sc.desc()
    assert L.rt_scene_upload(ctx, C.byref(d)) == A.RT_OK
    assert L.rt_resolve_hits(ctx, vp(r), vp(h), 8, vp(s), vp(m)) == A.RT_ERR_STATE   # no tree yet
    assert L.rt_resolve_hits_on(ctx, vp(r), vp(h), 8, vp(s), None, None) == A.RT_ERR_STATE
    assert b"rt_bvh_build" in L.rt_last_error(ctx)
    assert L.rt_bvh_build(ctx) == A.RT_OK
    assert L.rt_resolve_hits(ctx, vp(r), vp(h), 8, vp(s), vp(m)) == A.RT_OK   # no rt_resize needed
    E = A.RT_ERR_INVALID_ARG
    assert L.rt_resolve_hits(ctx, vp(r + 4), vp(h), 7, vp(s), vp(m)) == E
    assert L.rt_resolve_hits(ctx, vp(r), vp(h + 8), 7, vp(s), vp(m)) == E
    assert L.rt_resolve_hits(ctx, vp(r), vp(h), 7, vp(s + 4), vp(m)) == E
    assert L.rt_resolve_hits(ctx, vp(r), vp(h), 7, vp(s), vp(m + 8)) == E
    assert L.rt_resolve_hits(ctx, None, vp(h), 8, vp(s), vp(m)) == E
    assert L.rt_resolve_hits(ctx, vp(r), None, 8, vp(s), vp(m)) == E
    assert L.rt_resolve_hits_on(ctx, vp(r), vp(h), 8, None, vp(m), None) == E
    assert L.rt_resolve_hits(ctx, vp(r + 32), vp(h + 32), 7, vp(s + 64), vp(m + 48)) == A.RT_OK   # 16-byte aligned is enough
    assert L.rt_resolve_hits(ctx, None, None, 0, None, None) == A.RT_OK   # n = 0: nothing launched
    assert L.rt_resolve_hits_on(ctx, None, None, 0, None, None, None) == A.RT_OK
    qs = A.QueryStats()
    assert L.rt_get_query_stats(ctx, C.byref(qs)) == A.RT_OK and qs.queries_total == 0
    assert L.rt_wait(ctx) == A.RT_OK
    assert L.rt_destroy(ctx) == A.RT_OK
    # the Python layer checks its tensors
    R = rt.Renderer(sc, 16, 16)
    for bad in (dict(rays=rays[:, :6]), dict(hits=hits[:4]), dict(hits=hits.to(torch.float64)), dict(out=mat),
                dict(out=(surf, surf)), dict(rays=rays.cpu().numpy()), dict(out=surf.view(torch.int32))):
        kw = dict(rays=rays, hits=hits)
        kw.update(bad)
        with pytest.raises(ValueError):
            R.resolve(**kw)
    R.close()


def test_resolve_host_array_path(rt, orc, assets):
    c = surface_case(rt, orc, assets, "c3g", 600)
    R = rt.Renderer(c["scene"], 16, 16, pipeline="megakernel")
    h = R.trace(c["rays"])
    S = R.resolve(c["rays"], h)
    assert isinstance(S.buffer, np.ndarray) and S.normal.dtype == np.float32 and S.flags.dtype == np.int32
    assert len(S) == 604 and S.uv.shape == (604, 2) and S.position.shape == (604, 3)
    _assert_buffers((S.buffer, S.material_buffer), c["host"])
    R.close()


# ---- 10. one bounce in torch ---------------------------------------------------------------------------------
def test_one_bounce_in_torch(rt, orc, assets):
    """trace -> resolve -> (torch makes the next rays) -> trace_any: ambient-occlusion rays from
    the resolved C1 camera hits; the occlusion words equal the host tracer's on the same rays."""
    import torch
    sc = rt.Scene.preset("c1", assets)
    o, d = sr.camera_rays(rt, orc, 96, 64, 21)
    R = rt.Renderer(sc, 16, 16)
    rays = _device_rays(rt, o, d)
    # everything on torch's default stream (HIP's null stream): each step is ordered after the one before
    S = R.resolve(rays, R.trace(rays, stream=0), material=False, stream=0)
    hit = S.triangle != -1
    P, N = S.position[hit], S.normal[hit]
    g = torch.Generator(device="cuda:0").manual_seed(3)
    u1 = torch.rand(P.shape[0], generator=g, device="cuda:0")
    u2 = torch.rand(P.shape[0], generator=g, device="cuda:0")
    axis = torch.tensor([0.0072, 1.0, 0.0034], device="cuda:0").expand_as(N)
    T = torch.nn.functional.normalize(torch.cross(N, axis, dim=1), dim=1)
    B = torch.cross(T, N, dim=1)
    r, phi = torch.sqrt(u1), 2 * np.pi * u2
    D = (r * torch.cos(phi))[:, None] * T + (r * torch.sin(phi))[:, None] * B + torch.sqrt(1 - u1)[:, None] * N
    O = P + N * 1e-3
    ao = rt.Renderer.make_rays(O, D)
    occ = R.trace(ao, any_hit=True, stream=0)
    torch.cuda.synchronize()
    R.wait()
    rec = ao.cpu().numpy()
    assert rec.shape[0] == int(hit.sum().item()) > 0
    ref = rt.debug_trace_host(sc, rec[:, 0:3], rec[:, 4:7], any_hit=True)["id"] != MISS
    assert np.array_equal(occ.cpu().numpy(), ref.astype(np.int32))
    assert 0 < ref.sum() < len(ref)
    R.close()
