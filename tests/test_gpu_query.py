"""Device ray queries (Renderer.trace -> rt_trace_closest / rt_trace_any, csrc/rt_query.hip): the
caller's rays traced on the GPU against the built scene.

Closest-hit records must equal the library's host tracer (rt_debug_trace_host: the same traversal
code compiled for the host) bit for bit, and the CPU oracle on a prefix; any-hit must report the same
occlusion.  Rays are those of tests/test_bvh_host.py (_rays) plus its four axis-parallel and
pointing-away rays."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MISS = 0xFFFFFFFF
SCENES = [("c1", 3000), ("c2", 1500), ("c3g", 600)]


def _rays(rng, n):
    # tests/test_bvh_host.py::_rays: from points around the scene toward random points inside its bounds
    lo, hi = np.array([-3.0, -0.5, -2.0]), np.array([4.0, 3.0, 4.0])
    o = rng.uniform(lo, hi, size=(n, 3)).astype(np.float32)
    tgt = rng.uniform(lo, hi, size=(n, 3)).astype(np.float32)
    d = tgt - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return o, d.astype(np.float32)


def _edge_rays():
    # tests/test_bvh_host.py::test_empty_and_parallel_rays: zero direction components, and away from everything
    o = np.array([[0, 5, 0], [0, 0.5, 10], [0, 0.5, 10], [100, 100, 100]], np.float32)
    d = np.array([[0, -1, 0], [0, 0, -1], [0, 0, 1], [1, 0, 0]], np.float32)
    return o, d


def _batch(seed, n):
    """n random rays followed by the four edge rays."""
    o, d = _rays(np.random.default_rng(seed), n)
    eo, ed = _edge_rays()
    return np.concatenate([o, eo]), np.concatenate([d, ed])


# One scene, ray batch and host reference per preset, computed once and shared (never modified).
_CACHE = {}


def _case(rt, assets, preset, n):
    key = (preset, n)
    if key not in _CACHE:
        if preset == "c1+train":   # a mesh of six submeshes (the train) in the C1 room
            sc = rt.Scene.preset("c1", assets)
            sc.add_model(os.path.join(assets, "train.obj"), (-0.3, 0.0, 0.4), scale=0.5)
        else:
            sc = rt.Scene.preset(preset, assets)
        o, d = _batch(5, n)
        _CACHE[key] = dict(scene=sc, o=o, d=d, ref=rt.debug_trace_host(sc, o, d))
    return _CACHE[key]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _to_np(h):
    return {k: getattr(h, k).cpu().numpy() for k in ("t", "u", "v", "triangle", "mesh", "submesh", "primitive")}


def _assert_closest(got, ref, what=""):
    """got: dict of numpy arrays from a Hits; ref: rt.debug_trace_host output (same length)."""
    assert np.array_equal(got["triangle"].view(np.uint32), ref["id"]), what
    for k in ("t", "u", "v"):
        assert np.array_equal(_bits(got[k]), _bits(ref[k])), (what, k)


def _device_rays(rt, o, d, tmax=None):
    import torch
    r = torch.from_numpy(rt.Renderer.make_rays(o, d, tmax)).to("cuda:0")
    torch.cuda.synchronize()
    return r


def _trace_np(R, rays, **kw):
    import torch
    h = R.trace(rays, **kw)
    R.wait()
    torch.cuda.synchronize()
    return h.cpu().numpy() if kw.get("any_hit") else _to_np(h)


def _owners(desc):
    """mesh, submesh and primitive of every scene-wide triangle id, from the submesh index counts."""
    mesh, sub, prim = [], [], []
    for m in range(desc.mesh_count):
        md = desc.meshes[m]
        for s in range(md.submesh_count):
            k = md.submeshes[s].index_count // 3
            mesh += [m] * k
            sub += [s] * k
            prim += range(k)
    return np.array(mesh, np.int32), np.array(sub, np.int32), np.array(prim, np.int32)


def _desc_with(rt, desc, mesh, positions=None, normals=None, transform=None):
    """A copy of desc whose mesh `mesh` points at other positions / normals / transform
    (tests/test_gpu_dynamic.py::_desc_with)."""
    A = rt._abi
    arr = (A.MeshDesc * desc.mesh_count)()
    for m in range(desc.mesh_count):
        C.pointer(arr[m])[0] = desc.meshes[m]
    md = arr[mesh]
    if positions is not None:
        md.positions = C.cast(positions.ctypes.data, C.POINTER(A.Float3))
    if normals is not None:
        md.normals = C.cast(normals.ctypes.data, C.POINTER(A.Float3))
    if transform is not None:
        C.memmove(C.byref(md.transform), np.ascontiguousarray(transform, np.float32).ctypes.data, 48)
    d = A.SceneDesc()
    d.mesh_count, d.light_count, d.meshes, d.lights = desc.mesh_count, desc.light_count, arr, desc.lights
    d.texture_count, d.textures = desc.texture_count, desc.textures
    d._keep = (arr, positions, normals)
    return d


class _DescScene:
    """A scene descriptor built in the test, for debug_trace_host (which only calls desc())."""

    def __init__(self, d):
        self._d = d

    def desc(self):
        return self._d


# ---- 1. closest hit, bitwise ----------------------------------------------------------------------
@pytest.mark.parametrize("preset,n", SCENES)
def test_closest_hit_bitwise(rt, orc, assets, preset, n):
    c = _case(rt, assets, preset, n)
    R = rt.Renderer(c["scene"], 16, 16)
    got = _trace_np(R, _device_rays(rt, c["o"], c["d"]))
    _assert_closest(got, c["ref"], preset)
    qs = R.query_stats()
    assert qs.rays == n + 4 and qs.hits == int((c["ref"]["id"] != MISS).sum()) and qs.any_hit == 0
    assert 0 < qs.hits < qs.rays   # the batch holds hits and misses
    assert qs.grid_blocks == (n + 4 + 255) // 256   # a small batch does not launch the whole chip
    assert qs.queries_total == 1 and qs.total_rays == qs.rays and qs.device_ms > 0
    assert qs.node_visits == 0 and qs.tri_tests == 0   # counting is off
    # the first 300 rays (and the four edge rays) against the CPU oracle
    o_s = orc.OracleScene(c["scene"].desc())
    for k in list(range(300)) + list(range(n, n + 4)):
        ref = o_s.intersect(c["o"][k], c["d"][k])
        if ref is None:
            assert got["triangle"][k] == -1 and np.isinf(got["t"][k]), k
            continue
        t, i, u, v = ref
        assert got["triangle"][k] == i and got["t"][k] == np.float32(t), k
        assert got["u"][k] == np.float32(u) and got["v"][k] == np.float32(v), k
    R.close()


@pytest.mark.parametrize("n", [1, 63, 65])
def test_closest_hit_partial_waves_and_chunks(rt, assets, n):
    """Batches of 1, 63 and 65 rays (3000 + 4: test_closest_hit_bitwise): a partial wave, a partial
    chunk, and one ray past a chunk."""
    c = _case(rt, assets, "c1", 3000)
    R = rt.Renderer(c["scene"], 16, 16)
    got = _trace_np(R, _device_rays(rt, c["o"][:n], c["d"][:n]))
    _assert_closest(got, {k: v[:n] for k, v in c["ref"].items()}, n)
    assert R.query_stats().rays == n and R.query_stats().grid_blocks == 1
    R.close()


# ---- 2. refill path ---------------------------------------------------------------------------------
def test_refill_path_large_batch(rt, assets):
    """More rays than the launch has lanes: every lane refills from the chunk counters."""
    n = (1 << 20) + 37
    sc = rt.Scene.preset("c1", assets)
    o, d = _rays(np.random.default_rng(11), n)
    ref = rt.debug_trace_host(sc, o, d)
    R = rt.Renderer(sc, 16, 16)
    got = _trace_np(R, _device_rays(rt, o, d))
    qs = R.query_stats()
    assert qs.grid_blocks * 256 < n, qs.grid_blocks
    assert qs.rays == n and qs.hits == int((ref["id"] != MISS).sum())
    _assert_closest(got, ref)
    R.close()


# ---- 3. ownership -----------------------------------------------------------------------------------
@pytest.mark.parametrize("preset,n", SCENES + [("c1+train", 2000)])
def test_ownership_and_miss_record(rt, assets, preset, n):
    c = _case(rt, assets, preset, n)
    R = rt.Renderer(c["scene"], 16, 16)
    h = R.trace(_device_rays(rt, c["o"], c["d"]))
    R.wait()
    got = _to_np(h)
    raw = h.buffer.cpu().numpy().view(np.uint32)
    mesh, sub, prim = _owners(c["scene"].desc())
    assert len(mesh) == c["scene"].triangle_count
    hit = c["ref"]["id"] != MISS
    ids = c["ref"]["id"][hit].astype(np.int64)
    assert np.array_equal(got["mesh"][hit], mesh[ids])
    assert np.array_equal(got["submesh"][hit], sub[ids])
    assert np.array_equal(got["primitive"][hit], prim[ids])
    assert len(set(got["mesh"][hit])) > 1   # several meshes are hit
    if preset == "c1+train":
        assert len(set(got["submesh"][hit])) > 2 and got["primitive"][hit & (got["submesh"] > 0)].max() > 0
    # a miss record is exactly (inf, 0, 0, -1, -1, -1, -1, 0); a hit's reserved word is 0
    miss = np.array([np.float32(np.inf).view(np.uint32), 0, 0, MISS, MISS, MISS, MISS, 0], np.uint32)
    assert (~hit).any() and np.array_equal(raw[~hit], np.broadcast_to(miss, raw[~hit].shape))
    assert np.all(raw[hit, 7] == 0)
    R.close()


# ---- 4. any hit -------------------------------------------------------------------------------------
@pytest.mark.parametrize("preset", ["c1", "c2"])
def test_any_hit(rt, orc, assets, preset):
    sc = rt.Scene.preset(preset, assets)
    rng = np.random.default_rng(9)
    n = 800
    o, d = _rays(rng, n)
    eo, ed = _edge_rays()
    o, d = np.concatenate([o, eo]), np.concatenate([d, ed])
    tmax = rng.uniform(0.1, 6.0, size=n + 4).astype(np.float32)
    ref = rt.debug_trace_host(sc, o, d, tmax=tmax, any_hit=True)["id"] != MISS
    R = rt.Renderer(sc, 16, 16)
    occ = _trace_np(R, _device_rays(rt, o, d, tmax), any_hit=True)
    assert occ.dtype == np.int32 and occ.shape == (n + 4,)
    assert np.array_equal(occ, ref.astype(np.int32))
    assert 0 < ref.sum() < n
    qs = R.query_stats()
    assert qs.any_hit == 1 and qs.rays == n + 4 and qs.hits == int(ref.sum())
    o_s = orc.OracleScene(sc.desc())
    for k in range(200):
        assert (o_s.intersect(o[k], d[k], tmax=float(tmax[k]), any_hit=True) is not None) == bool(occ[k]), k
    # closest hit honours tmax too: the hit within [0, tmax], else a miss
    got = _trace_np(R, _device_rays(rt, o, d, tmax))
    _assert_closest(got, rt.debug_trace_host(sc, o, d, tmax=tmax))
    R.close()


# ---- 5. device-built tree ---------------------------------------------------------------------------
@pytest.mark.parametrize("preset,n", [("c2", 1500), ("c3g", 600)])
def test_device_built_tree(rt, assets, preset, n):
    c = _case(rt, assets, preset, n)
    R = rt.Renderer(c["scene"], 16, 16, bvh="lbvh")
    got = _trace_np(R, _device_rays(rt, c["o"], c["d"]))
    _assert_closest(got, c["ref"], preset)
    mesh, sub, prim = _owners(c["scene"].desc())
    hit = c["ref"]["id"] != MISS
    assert np.array_equal(got["primitive"][hit], prim[c["ref"]["id"][hit].astype(np.int64)])
    tmax = np.random.default_rng(3).uniform(0.1, 6.0, size=n + 4).astype(np.float32)
    ref_any = rt.debug_trace_host(c["scene"], c["o"], c["d"], tmax=tmax, any_hit=True)["id"] != MISS
    occ = _trace_np(R, _device_rays(rt, c["o"], c["d"], tmax), any_hit=True)
    assert np.array_equal(occ, ref_any.astype(np.int32))
    R.close()


# ---- 6. counting ------------------------------------------------------------------------------------
def test_counting_matches_host_walk(rt, assets):
    """With counting on, a closest-hit batch on the host SAH tree visits the nodes and tests the
    triangles the host tracer does: the same tree (the same builder on the same world-space
    triangles), the same order and the same bound (the closest hit so far).

    The two walks may differ in single box tests, though: the device forms the slab reciprocals
    1 / d with the hardware's 1-ulp reciprocal, the host with a correctly rounded division
    (ray_setup, rt_device.h; the boxes are padded, so results do not depend on it).  A box test
    flips only where a slab interval is empty or not by an ulp or so of its bounds (a fraction of
    the order of 1e-6 of the ~5e4 box tests of this batch), and a flip adds or removes one subtree
    visit.  So the sums are asserted to 1e-3 relative (six node visits of ~6000): room for a few
    such flips, far below what a wrong bound, order or tree costs (percent and more).  Hits, which
    do not depend on it, are exact."""
    c = _case(rt, assets, "c2", 1500)
    R = rt.Renderer(c["scene"], 16, 16)
    R.set_counting(True)
    got = _trace_np(R, _device_rays(rt, c["o"], c["d"]))
    _assert_closest(got, c["ref"])
    qs = R.query_stats()
    want_n, want_t = int(c["ref"]["nodes"].astype(np.int64).sum()), int(c["ref"]["tris"].astype(np.int64).sum())
    print(f"query counting: nodes {qs.node_visits} (host {want_n}), triangles {qs.tri_tests} (host {want_t})")
    assert abs(int(qs.node_visits) - want_n) <= 1e-3 * want_n, (qs.node_visits, want_n)
    assert abs(int(qs.tri_tests) - want_t) <= 1e-3 * want_t, (qs.tri_tests, want_t)
    assert qs.total_node_visits == qs.node_visits
    R.set_counting(False)
    _trace_np(R, _device_rays(rt, c["o"][:100], c["d"][:100]))
    qs = R.query_stats()
    assert qs.node_visits == 0 and qs.queries_total == 2 and qs.total_rays == 1504 + 100
    R.close()


# ---- 7. dynamic geometry ----------------------------------------------------------------------------
def test_query_then_update_then_query(rt, assets):
    """A query enqueued before a geometry update sees the old geometry, one after it the new: the
    update waits for the pending query before it rewrites the generation in place."""
    import torch
    c = _case(rt, assets, "c2", 1500)
    sc, desc = c["scene"], c["scene"].desc()
    R = rt.Renderer(sc, 16, 16)
    rays = _device_rays(rt, c["o"], c["d"])
    h0 = R.trace(rays)   # not waited for
    mats = np.stack([np.frombuffer(bytes(desc.meshes[k].transform), np.float32).reshape(4, 3).copy()
                     for k in range(desc.mesh_count)])
    mats[0, 3, 0] += 0.35
    R.set_instance_transforms(mats)
    R.refit()
    h1 = R.trace(rays)
    R.wait()
    torch.cuda.synchronize()
    _assert_closest(_to_np(h0), c["ref"], "before the update")
    moved = _DescScene(_desc_with(rt, desc, 0, transform=mats[0]))
    ref1 = rt.debug_trace_host(moved, c["o"], c["d"])
    assert not np.array_equal(ref1["id"], c["ref"]["id"])   # the move changes what some rays hit
    _assert_closest(_to_np(h1), ref1, "after the update")
    # ... and once more after a frame has made the new generation current, and after a rebuild
    R.draw()
    _assert_closest(_trace_np(R, rays), ref1, "after a frame")
    R.rebuild()
    _assert_closest(_trace_np(R, rays), ref1, "after a rebuild")
    R.close()


# ---- 8. streams and frames --------------------------------------------------------------------------
def test_two_streams_back_to_back(rt, assets):
    import torch
    c = _case(rt, assets, "c1", 3000)
    R = rt.Renderer(c["scene"], 16, 16)
    ra = _device_rays(rt, c["o"][:2000], c["d"][:2000])
    rb = _device_rays(rt, c["o"][1000:], c["d"][1000:])
    outs = [torch.empty((r.shape[0], 8), dtype=torch.float32, device="cuda:0") for r in (ra, rb, ra, rb)]
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    hs = [R.trace(ra, out=outs[0], stream=s1.cuda_stream), R.trace(rb, out=outs[1], stream=s2.cuda_stream),
          R.trace(ra, out=outs[2], stream=s2.cuda_stream), R.trace(rb, out=outs[3], stream=0)]
    s1.synchronize()
    s2.synchronize()
    torch.cuda.synchronize()
    refa = {k: v[:2000] for k, v in c["ref"].items()}
    refb = {k: v[1000:] for k, v in c["ref"].items()}
    for h, ref in zip(hs, (refa, refb, refa, refb)):
        _assert_closest(_to_np(h), ref)
    assert R.query_stats().queries_total == 4
    R.close()


def test_frames_unchanged_by_interleaved_queries(rt, assets):
    import torch
    c = _case(rt, assets, "c2", 1500)
    rays = _device_rays(rt, c["o"], c["d"])
    side = torch.cuda.Stream()

    def run(with_queries):
        R = rt.Renderer(c["scene"], 96, 64, seed=4, frames_in_flight=4)
        R.samplesPerPixel = 2
        R.maxBounces = 3
        hs, frames = [], []
        for f in range(3):
            if with_queries:
                hs.append(R.trace(rays))
            R.draw()
            if with_queries:
                hs.append(R.trace(rays, stream=side.cuda_stream))
                hs.append(R.trace(rays, any_hit=True))
        out = (R.radiance(), *R.aux()[:2])
        # ... and again with every frame read back
        for f in range(3):
            if with_queries:
                hs.append(R.trace(rays))
            R.draw()
            frames.append(R.radiance())
        side.synchronize()
        for h in hs:
            if isinstance(h, rt.Hits):
                _assert_closest(_to_np(h), c["ref"])
        R.close()
        return out, frames

    (rad0, dep0, mot0), fr0 = run(False)
    (rad1, dep1, mot1), fr1 = run(True)
    assert np.array_equal(rad0, rad1) and np.array_equal(dep0, dep1) and np.array_equal(mot0, mot1)
    for a, b in zip(fr0, fr1):
        assert np.array_equal(a, b)
    assert rad0[..., :3].max() > 0


# ---- 9. errors --------------------------------------------------------------------------------------
def test_query_errors(rt, assets):
    import torch
    A, L = rt._abi, rt.lib()
    sc = rt.Scene.preset("c1", assets)
    rays = _device_rays(rt, *_edge_rays())
    hits = torch.empty((4, 8), dtype=torch.float32, device="cuda:0")
    occ = torch.empty((4,), dtype=torch.int32, device="cuda:0")
    vp = C.c_void_p
    # a context with the scene uploaded only: no tree to trace
    ctx = vp()
    assert L.rt_create(C.byref(A.Opts()), C.byref(ctx)) == A.RT_OK
    d = sc.desc()
    assert L.rt_scene_upload(ctx, C.byref(d)) == A.RT_OK
    assert L.rt_trace_closest(ctx, vp(rays.data_ptr()), 4, vp(hits.data_ptr())) == A.RT_ERR_STATE
    assert L.rt_trace_any(ctx, vp(rays.data_ptr()), 4, vp(occ.data_ptr())) == A.RT_ERR_STATE
    assert b"rt_bvh_build" in L.rt_last_error(ctx)
    assert L.rt_bvh_build(ctx) == A.RT_OK
    assert L.rt_trace_closest(ctx, vp(rays.data_ptr()), 4, vp(hits.data_ptr())) == A.RT_OK   # no rt_resize needed
    # misaligned and NULL pointers
    E = A.RT_ERR_INVALID_ARG
    assert L.rt_trace_closest(ctx, vp(rays.data_ptr() + 4), 3, vp(hits.data_ptr())) == E
    assert L.rt_trace_closest(ctx, vp(rays.data_ptr()), 3, vp(hits.data_ptr() + 8)) == E
    assert L.rt_trace_any(ctx, vp(rays.data_ptr()), 3, vp(occ.data_ptr() + 2)) == E
    assert L.rt_trace_any(ctx, vp(rays.data_ptr()), 3, vp(occ.data_ptr() + 4)) == A.RT_OK   # 4-byte aligned is enough
    assert L.rt_trace_closest(ctx, None, 4, vp(hits.data_ptr())) == E
    assert L.rt_trace_any_on(ctx, vp(rays.data_ptr()), 4, None, None) == E
    # n = 0: RT_OK, nothing launched
    before = A.QueryStats()
    assert L.rt_get_query_stats(ctx, C.byref(before)) == A.RT_OK
    assert L.rt_trace_closest(ctx, None, 0, None) == A.RT_OK
    assert L.rt_trace_any_on(ctx, None, 0, None, None) == A.RT_OK
    after = A.QueryStats()
    assert L.rt_get_query_stats(ctx, C.byref(after)) == A.RT_OK
    assert after.queries_total == before.queries_total == 2
    assert L.rt_wait(ctx) == A.RT_OK
    assert L.rt_destroy(ctx) == A.RT_OK
    # the Python layer checks its tensors
    R = rt.Renderer(sc, 16, 16)
    with pytest.raises(ValueError):
        R.trace(rays[:, :6])
    with pytest.raises(ValueError):
        R.trace(rays, out=occ)
    R.close()


# ---- 10. host-array path ----------------------------------------------------------------------------
def test_host_array_path(rt, assets):
    c = _case(rt, assets, "c1", 3000)
    R = rt.Renderer(c["scene"], 16, 16, pipeline="megakernel")   # queries need only the geometry and the tree
    rays = rt.Renderer.make_rays(c["o"], c["d"])
    h = R.trace(rays)
    assert isinstance(h.t, np.ndarray) and h.t.dtype == np.float32 and h.triangle.dtype == np.int32
    assert len(h) == 3004 and h.buffer.shape == (3004, 8)
    dev = _trace_np(R, _device_rays(rt, c["o"], c["d"]))
    for k in ("t", "u", "v"):
        assert np.array_equal(_bits(getattr(h, k)), _bits(dev[k])), k
    for k in ("triangle", "mesh", "submesh", "primitive"):
        assert np.array_equal(getattr(h, k), dev[k]), k
    _assert_closest({k: getattr(h, k) for k in ("t", "u", "v", "triangle")}, c["ref"])
    tmax = np.full(3004, 2.5, np.float32)
    occ = R.trace(rt.Renderer.make_rays(c["o"], c["d"], tmax), any_hit=True)
    assert isinstance(occ, np.ndarray) and occ.dtype == np.int32
    ref = rt.debug_trace_host(c["scene"], c["o"], c["d"], tmax=tmax, any_hit=True)["id"] != MISS
    assert np.array_equal(occ, ref.astype(np.int32))
    R.close()
