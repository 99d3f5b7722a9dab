"""Shading queries on the device (Renderer.shade -> rt_shade_hits, rq_shade in csrc/rt_query.hip).

The records must equal the host hook's (rt_debug_shade_host: the same scatter_eval compiled for the
host) and, run as the loop trace -> resolve -> shade -> trace_any + trace -> ..., re-assemble the
frame rt_render_frame renders, radiance and ray counts.  Every comparison is bitwise.  Scenes,
records and host references are those of tests/test_shade_host.py.

No test here gives the device anything it does not handle by design: bad arguments are rejected on
the host before any launch."""
import ctypes as C

import numpy as np
import pytest

import shade_ref as sh
import surface_ref as sr
from helpers import make_light, make_renderer, textured_scene
from test_shade_host import SEED, assert_shaded_equal, same, shade_case, take

pytestmark = pytest.mark.gpu
F = np.float32


def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


def _np(x):
    return x.cpu().numpy()


def _surface(rt, S):
    import torch
    s, m = _dev(S.buffer), _dev(S.material_buffer)
    return rt.Surface(s, s.view(torch.int32), m, m.view(torch.int32))


def _shade_np(rt, R, rays, S, paths, randoms=None, **kw):
    """Renderer.shade on device copies of host records; the results as a Shaded of numpy arrays."""
    import torch
    p = _dev(paths)
    args = (_dev(rays), _surface(rt, S), p)
    torch.cuda.synchronize()
    out = R.shade(*args, randoms=None if randoms is None else _dev(randoms), **kw)
    R.wait()
    torch.cuda.synchronize()
    assert out.paths.buffer.data_ptr() == p.data_ptr()   # in place
    pn = _np(p)
    return rt.Shaded(rt.Paths(pn, pn.view(np.int32)), _np(out.next_rays), _np(out.shadow_rays), _np(out.contrib))


def _mixed(c, limit=4000):
    """A few thousand of a case's mid-loop records with every ninth path killed: mixed bounce /
    step / dead states."""
    rays, S, paths = take(c, slice(None, None, -(-len(c["paths"]) // limit)))
    paths = paths.copy()
    paths.view(np.uint32)[::9, 7] &= ~np.uint32(sh.ALIVE)
    return rays, S, paths


# ---- 1. device against the host hook ---------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c1", "textured", "glass"])
def test_device_shade_equals_host(rt, orc, assets, name):
    c = shade_case(rt, orc, assets, name)
    B = c["backend"]
    rays, S, paths = _mixed(c)
    P = rt.Paths(paths, paths.view(np.int32))
    print(f"{name}: {len(paths)} records, steps 0..{P.step.max()}, {(~P.alive).sum()} dead, "
          f"{(S.triangle == -1).sum()} misses")
    assert P.step.max() > 0 and P.alive.any() and (~P.alive).any()
    R = rt.Renderer(c["scene"], 16, 16)
    opts = dict(shading_mode=c["mode"], max_bounces=c["max_bounces"])
    before = R.query_stats().queries_total
    assert_shaded_equal(_shade_np(rt, R, rays, S, paths, **opts), B.shade(rays, S, paths), name)
    rnd = np.random.default_rng(11).random((len(paths), 8)).astype(F)
    rnd[:, 6:] = 0
    assert_shaded_equal(_shade_np(rt, R, rays, S, paths, randoms=rnd, **opts), B.shade(rays, S, paths, randoms=rnd), name)
    assert R.query_stats().queries_total == before   # a shade is not a query of rt_query_stats
    R.close()


@pytest.mark.parametrize("n", [1, 63, 65])
def test_device_shade_partial_waves(rt, orc, assets, n):
    c = shade_case(rt, orc, assets, "textured")
    rays, S, paths = take(c, slice(100, 100 + n))
    R = rt.Renderer(c["scene"], 16, 16)
    opts = dict(shading_mode=c["mode"], max_bounces=c["max_bounces"])
    assert_shaded_equal(_shade_np(rt, R, rays, S, paths, **opts), c["backend"].shade(rays, S, paths), n)
    R.close()


# ---- 2. the query integrator against the frame --------------------------------------------------------------
FRAMES = {
    "c1": ("c1", 96, 64, 2, 4, 0),
    "c1-legacy": ("c1", 64, 48, 2, 3, 1),
    "textured": ("textured", 96, 64, 1, 3, 0),
    "c3g": ("c3g", 96, 54, 2, 8, 0),
}


@pytest.mark.parametrize("pipeline", ["megakernel", "wavefront"])
@pytest.mark.parametrize("name", list(FRAMES))
def test_query_integrator_equals_frame(rt, orc, assets, name, pipeline):
    """Frame 0 re-assembled from queries on the device (torch tensors on one stream, dead records
    carried, shadow rays compacted by a boolean index, torch.where for the add) against the frame
    the same Renderer draws; and that frame against one a Renderer draws without any query."""
    import torch
    what, W, H, spp, mb, mode = FRAMES[name]
    sc = textured_scene(rt, assets) if what == "textured" else rt.Scene.preset(what, assets)

    def renderer():
        R = make_renderer(rt, sc, W, H, pipeline, seed=SEED)
        R.samplesPerPixel, R.maxBounces, R.shadingMode = spp, mb, mode
        return R

    R = renderer()
    got = sh.render(sh.DeviceBackend(rt, R), rt, orc, W, H, SEED, spp, mb, compact=False, to_backend=_dev)
    torch.cuda.synchronize()
    R.draw()
    R.wait()
    frame, st = R.radiance(), R.stats()
    print(f"{name} {pipeline}: {got['closest_rays']} closest rays, {got['shadow_rays']} shadow rays, {got['paths']} paths")
    assert (got["closest_rays"], got["shadow_rays"], got["paths"]) == (st.closest_rays, st.shadow_rays, st.paths)
    assert same(got["radiance"], frame[..., :3]) and got["radiance"].any()
    R.close()
    R2 = renderer()
    R2.draw()
    R2.wait()
    assert same(R2.radiance(), frame)   # the queries did not disturb the frame
    R2.close()


# ---- 3. lights follow the upload --------------------------------------------------------------------------------
def test_lights_follow_the_upload(rt, orc, assets):
    c = shade_case(rt, orc, assets, "c1")
    rays, S, paths = take(c, slice(0, 2000))
    sc = rt.Scene.preset("c1", assets)
    lights0 = sh.scene_lights(sc)
    R = rt.Renderer(sc, 16, 16)
    opts = dict(shading_mode=0, max_bounces=4)
    first = _shade_np(rt, R, rays, S, paths, light_count=0, **opts)
    lights1 = [make_light(rt, k) for k in ("spot", "point", "sun")]
    sc.set_lights(lights1)
    R.upload(sc.desc())
    second = _shade_np(rt, R, rays, S, paths, light_count=0, **opts)
    assert_shaded_equal(first, rt.debug_shade_host(lights0, rays, S, paths, **opts), "before")
    assert_shaded_equal(second, rt.debug_shade_host(lights1, rays, S, paths, **opts), "after")
    assert not same(first.shadow_rays, second.shadow_rays)
    R.close()


# ---- 4. plumbing ---------------------------------------------------------------------------------------------------
def test_shade_streams_out_buffers_and_aliasing(rt, orc, assets):
    import torch
    c = shade_case(rt, orc, assets, "textured")
    B = c["backend"]
    R = rt.Renderer(c["scene"], 16, 16)
    opts = dict(shading_mode=c["mode"], max_bounces=c["max_bounces"])
    batches = [take(c, slice(0, 1500)), take(c, slice(500, 2600))]
    want = [B.shade(*b) for b in batches]
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    streams = [s1.cuda_stream, s2.cuda_stream, s2.cuda_stream, 0, None, s1.cuda_stream]   # more shades in flight than slots
    ins = []
    for k in range(6):
        rays, S, paths = batches[k % 2]
        n = len(paths)
        # contrib sits inside a poisoned tensor, one record of poison on either side
        pad = torch.full((n + 2, 4), -123.25, dtype=torch.float32, device="cuda:0")
        out = (torch.empty((n, 8), dtype=torch.float32, device="cuda:0"), torch.empty((n, 8), dtype=torch.float32, device="cuda:0"),
               pad[1:n + 1])
        r = _dev(rays)
        if k == 2:
            out = (r, out[1], out[2])   # next_rays aliases rays
        ins.append((r, _surface(rt, S), _dev(paths), out, pad))
    before = R.query_stats().queries_total
    torch.cuda.synchronize()
    outs = [R.shade(r, S, p, out=out, stream=st, **opts) for (r, S, p, out, _), st in zip(ins, streams)]
    s1.synchronize()
    s2.synchronize()
    torch.cuda.synchronize()
    R.wait()
    for k, (o, (r, S, p, out, pad)) in enumerate(zip(outs, ins)):
        assert o.next_rays.data_ptr() == out[0].data_ptr() and o.contrib.data_ptr() == out[2].data_ptr()
        assert o.shadow_rays.data_ptr() == out[1].data_ptr() and o.paths.buffer.data_ptr() == p.data_ptr()
        pn = _np(p)
        got = rt.Shaded(rt.Paths(pn, pn.view(np.int32)), _np(o.next_rays), _np(o.shadow_rays), _np(o.contrib))
        assert_shaded_equal(got, want[k % 2], k)
        assert torch.all(pad[0] == -123.25).item() and torch.all(pad[-1] == -123.25).item(), k
    assert R.query_stats().queries_total == before
    R.close()


def test_shade_host_array_path(rt, orc, assets):
    c = shade_case(rt, orc, assets, "c1-legacy")
    rays, S, paths = take(c, slice(0, 700))
    R = rt.Renderer(c["scene"], 16, 16, pipeline="megakernel")
    R.shadingMode, R.maxBounces = c["mode"], c["max_bounces"]   # the options default to the uniforms
    keep = paths.copy()
    out = R.shade(rays, S, rt.Paths(paths, paths.view(np.int32)))
    assert isinstance(out.next_rays, np.ndarray) and isinstance(out.paths.buffer, np.ndarray) and len(out) == 700
    assert same(paths, keep)   # the host path leaves the given records alone
    assert_shaded_equal(out, c["backend"].shade(rays, S, paths))
    R.close()


def test_shade_errors(rt, orc, assets):
    import torch
    A, L = rt._abi, rt.lib()
    c = shade_case(rt, orc, assets, "c1")
    rays, S, paths = take(c, slice(0, 8))
    sc = c["scene"]
    t = dict(rays=_dev(rays), surfaces=_dev(S.buffer), materials=_dev(S.material_buffer), randoms=None, paths=_dev(paths),
             next_rays=torch.empty((8, 8), dtype=torch.float32, device="cuda:0"),
             shadow_rays=torch.empty((8, 8), dtype=torch.float32, device="cuda:0"),
             contrib=torch.empty((8, 4), dtype=torch.float32, device="cuda:0"))
    rnd = torch.zeros((8, 8), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    vp = C.c_void_p
    order = ("rays", "surfaces", "materials", "randoms", "paths", "next_rays", "shadow_rays", "contrib")
    size = dict(rays=32, surfaces=64, materials=48, randoms=32, paths=48, next_rays=32, shadow_rays=32, contrib=16)
    ptr = {k: (v.data_ptr() if v is not None else None) for k, v in t.items()}

    def call(ctx, opts=(0, 4, 0), n=8, on=False, **kw):
        a = dict(ptr)
        a.update(kw)
        op = A.ShadeOpts()
        op.shading_mode, op.max_bounces, op.light_count = opts
        args = [ctx, C.byref(op)] + [None if a[k] is None else vp(a[k]) for k in order[:4]] + [n] + \
               [None if a[k] is None else vp(a[k]) for k in order[4:]]
        return L.rt_shade_hits_on(*args, None) if on else L.rt_shade_hits(*args)

    ctx = vp()
    assert L.rt_create(C.byref(A.Opts()), C.byref(ctx)) == A.RT_OK
    assert call(ctx) == A.RT_ERR_STATE and call(ctx, on=True) == A.RT_ERR_STATE   # no scene yet
    assert b"rt_scene_upload" in L.rt_last_error(ctx)
    d = sc.desc()
    assert L.rt_scene_upload(ctx, C.byref(d)) == A.RT_OK
    assert call(ctx) == A.RT_OK and call(ctx, on=True) == A.RT_OK   # no tree, no rt_resize needed
    E = A.RT_ERR_INVALID_ARG
    assert L.rt_shade_hits(ctx, None, *[vp(ptr[k]) if ptr[k] else None for k in order[:4]], 8,
                           *[vp(ptr[k]) for k in order[4:]]) == E
    for k in order:
        if k != "randoms":
            assert call(ctx, **{k: None}) == E, k
            assert call(ctx, n=7, **{k: ptr[k] + 8}) == E, k
            assert call(ctx, n=7, **{k: ptr[k] + size[k]}) == A.RT_OK, k   # 16-byte aligned is enough
    assert call(ctx, randoms=rnd.data_ptr()) == A.RT_OK and call(ctx, n=7, randoms=rnd.data_ptr() + 4) == E
    for bad in ((2, 4, 0), (-1, 4, 0), (0, 0, 0), (0, 13, 0), (0, 4, -1), (0, 4, d.light_count + 1)):
        assert call(ctx, opts=bad) == E, bad
    assert call(ctx, opts=(1, 12, d.light_count)) == A.RT_OK
    assert call(ctx, n=0, **{k: None for k in order}) == A.RT_OK and call(ctx, n=0, on=True, **{k: None for k in order}) == A.RT_OK
    qs = A.QueryStats()
    assert L.rt_get_query_stats(ctx, C.byref(qs)) == A.RT_OK and qs.queries_total == 0
    assert L.rt_wait(ctx) == A.RT_OK
    assert L.rt_destroy(ctx) == A.RT_OK
    # the Python layer checks its tensors
    R = rt.Renderer(sc, 16, 16)
    Sd = _surface(rt, S)
    good = dict(rays=t["rays"], surface=Sd, paths=t["paths"])
    nomat = rt.Surface(Sd.buffer, Sd.buffer.view(torch.int32))
    for bad in (dict(rays=t["rays"][:, :6]), dict(rays=t["rays"][:4]), dict(paths=t["paths"].to(torch.float64)),
                dict(paths=t["paths"][:, :8]), dict(surface=nomat), dict(randoms=rnd[:, :4]), dict(randoms=rnd.cpu().numpy()),
                dict(rays=rays), dict(out=t["contrib"]), dict(out=(t["next_rays"], t["shadow_rays"], t["shadow_rays"])),
                dict(out=(t["next_rays"], t["shadow_rays"], t["contrib"].view(torch.int32)))):
        kw = dict(good)
        kw.update(bad)
        with pytest.raises(ValueError):
            R.shade(**kw)
    with pytest.raises(rt.RTError):
        R.shade(**good, light_count=R.light_count + 1)
    R.close()
