"""Path queries on the device (Renderer.camera_paths / compact / connect / retire / average /
path_trace -> rt_camera_paths .. rt_average_samples; rq_camera .. rq_compact_copy in
csrc/rt_query.hip).

The camera records must equal the host hook's, the compaction numpy's boolean indexing, connect /
retire / average their numpy statements, and the whole loop, run from library calls only, the frame
rt_render_frame renders: radiance in all four channels and the ray counts.  Every comparison is
bitwise.

No test here gives the device anything it does not handle by design: bad arguments are rejected on
the host before any launch."""
import ctypes as C

import numpy as np
import pytest

import surface_ref as sr
from helpers import make_renderer, textured_scene
from test_gpu_shade import FRAMES
from test_shade_host import SEED

pytestmark = pytest.mark.gpu
F = np.float32
ALIVE, SHADOW = 1, 2
POISON = 0xDEADBEEF
TILE = 1024   # kCompactTile of csrc/rt_paths.h: 300001 records are 293 tiles, the tile scan crosses waves and rounds


def same(a, b):
    return np.array_equal(sr.bits(a), sr.bits(b))


def _dev(x):
    import torch
    x = np.ascontiguousarray(x)
    if x.dtype == np.uint32:
        x = x.view(np.int32)
    return torch.from_numpy(x).to("cuda:0")


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.fixture(scope="module")
def R(rt, assets):
    r = rt.Renderer(rt.Scene.preset("c1", assets), 7, 5, seed=5)
    yield r
    r.close()


def _uniforms(rt, W, H, spp=2):
    u = rt.uniforms_default(W, H)
    u.camera = rt.camera_default(W, H)
    u.samplesPerPixel = spp
    return u


# ---- 4. camera paths on the device against the host hook ----------------------------------------------
def test_camera_full_image_equals_host(rt, R):
    import torch
    u = R.uniforms()
    for s, stride, off in ((0, 1, 0), (1, 2, 1)):
        want_r, want_p = rt.debug_camera_paths_host(u, R.random, s, tag_stride=stride, tag_offset=off)
        for rnd in (None, _dev(R.random), R.random):   # the context's own, the caller's, a host array
            torch.cuda.synchronize()
            rays, paths = R.camera_paths(s, random_offsets=rnd, tag_stride=stride, tag_offset=off)
            R.wait()
            assert same(rays.cpu().numpy(), want_r) and same(paths.buffer.cpu().numpy(), want_p.buffer)
    assert np.array_equal(_u32(paths.tag), np.arange(35, dtype=np.uint32) * 2 + 1)


@pytest.mark.parametrize("n", [1, 63, 65])
def test_camera_partial_waves(rt, R, n):
    import torch
    W, H, first = 11, 7, 5
    u = _uniforms(rt, W, H)
    u.frameIndex = 2
    rnd = rt.random_offsets(9, W, H)
    want_r, want_p = rt.debug_camera_paths_host(u, rnd, 1, first_pixel=first, n=n, tag_stride=3, tag_offset=2)
    pad_r = torch.full((n + 2, 8), -7.5, dtype=torch.float32, device="cuda:0")
    pad_p = torch.full((n + 2, 12), -7.5, dtype=torch.float32, device="cuda:0")
    d = _dev(rnd)
    torch.cuda.synchronize()
    rays, paths = R.camera_paths(1, first_pixel=first, n=n, uniforms=u, random_offsets=d, tag_stride=3, tag_offset=2,
                                 out=(pad_r[1:n + 1], pad_p[1:n + 1]), stream=0)
    torch.cuda.synchronize()
    assert rays.data_ptr() == pad_r[1:].data_ptr() and paths.buffer.data_ptr() == pad_p[1:].data_ptr()
    assert same(rays.cpu().numpy(), want_r) and same(paths.buffer.cpu().numpy(), want_p.buffer)
    for pad in (pad_r, pad_p):
        assert torch.all(pad[0] == -7.5).item() and torch.all(pad[-1] == -7.5).item()
    # the context's own offsets after rt_resize at this size
    R2 = rt.Renderer(R.scene, W, H, seed=9)
    rays2, paths2 = R2.camera_paths(1, first_pixel=first, n=n, uniforms=u, tag_stride=3, tag_offset=2)
    R2.wait()
    assert same(rays2.cpu().numpy(), want_r) and same(paths2.buffer.cpu().numpy(), want_p.buffer)
    R2.close()


def test_camera_errors(rt, R):
    u = _uniforms(rt, 11, 7)
    with pytest.raises(rt.RTError) as e:
        R.camera_paths(0, uniforms=u)   # NULL offsets, but the context's are 7 x 5
    assert e.value.code == rt._abi.RT_ERR_STATE
    for kw in (dict(first_pixel=30, n=6), dict(sample=-1), dict(tag_stride=0)):
        args = dict(sample=0)
        args.update(kw)
        with pytest.raises(rt.RTError) as e:
            R.camera_paths(**args)
        assert e.value.code == rt._abi.RT_ERR_INVALID_ARG, kw
    # after rt_create alone: no scene, no tree, no rt_resize, offsets given
    import torch
    A, L = rt._abi, rt.lib()
    ctx = C.c_void_p()
    assert L.rt_create(C.byref(A.Opts()), C.byref(ctx)) == A.RT_OK
    u = R.uniforms()
    o = A.CameraOpts()
    o.tag_stride = 1
    rnd = _dev(R.random)
    rays = torch.empty((35, 8), dtype=torch.float32, device="cuda:0")
    paths = torch.empty((35, 12), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    vp = C.c_void_p
    assert L.rt_camera_paths(ctx, C.byref(u), C.byref(o), None, 35, vp(rays.data_ptr()), vp(paths.data_ptr())) == A.RT_ERR_STATE
    assert L.rt_camera_paths(ctx, C.byref(u), C.byref(o), vp(rnd.data_ptr()), 35, vp(rays.data_ptr()), vp(paths.data_ptr())) == A.RT_OK
    assert L.rt_camera_paths(ctx, C.byref(u), C.byref(o), None, 0, None, None) == A.RT_ERR_STATE
    assert L.rt_camera_paths_on(ctx, C.byref(u), C.byref(o), vp(rnd.data_ptr()), 0, None, None, None) == A.RT_OK
    assert L.rt_wait(ctx) == A.RT_OK
    want_r, want_p = rt.debug_camera_paths_host(u, R.random, 0)
    assert same(rays.cpu().numpy(), want_r) and same(paths.cpu().numpy(), want_p.buffer)
    assert L.rt_destroy(ctx) == A.RT_OK


# ---- 5. compaction against numpy boolean indexing ------------------------------------------------------
SELECTIONS = ("none", "all", "first", "last", "ninth-cleared", "bernoulli")


def _selection(kind, n, rng):
    sel = np.zeros(n, bool)
    if kind == "all":
        sel[:] = True
    elif kind == "first":
        sel[0] = True
    elif kind == "last":
        sel[-1] = True
    elif kind == "ninth-cleared":
        sel[:] = True
        sel[::9] = False
    elif kind == "bernoulli":
        sel = rng.random(n) < 0.5
    return sel


def _records(n, sel, mask, rng):
    """Random bit patterns in every word (NaN patterns among them) of paths and of four streams of
    1, 2, 3 and 4 words (the 3-word one is the paths array itself); flags from {0, 1, 2, 3} such
    that exactly `sel` is selected by `mask`, with random bits above them that no mask looks at."""
    paths = rng.integers(0, 2 ** 32, (n, 12), dtype=np.uint32)
    paths[::5, 4] = 0x7FC00001   # NaNs with payloads
    paths[1::7, 0] = 0xFFFFFFFF
    yes = np.array([f for f in range(4) if f & mask], np.uint32)
    no = np.array([f for f in range(4) if not f & mask], np.uint32)
    flags = np.where(sel, yes[rng.integers(0, len(yes), n)], no[rng.integers(0, len(no), n)])
    paths[:, 7] = flags | (rng.integers(0, 2 ** 30, n, dtype=np.uint32) << 2)
    srcs = [rng.integers(0, 2 ** 32, (n, 4 * w), dtype=np.uint32) for w in (1, 2, 4)]
    return paths, srcs


def _check_compaction(rt, R, paths, srcs, mask, sel, what, stream=None):
    import torch
    n = len(paths)
    p = _dev(paths.view(F))
    tens = [_dev(srcs[0]), _dev(srcs[1]), p, _dev(srcs[2])]
    host = [srcs[0], srcs[1], paths, srcs[2]]
    want = np.nonzero(sel)[0].astype(np.uint32)
    m = len(want)
    first = None
    for rep in range(2):   # a second identical call gives identical output
        outs = [torch.full_like(t.view(torch.int32), POISON - 2 ** 32).view(t.dtype) for t in tens]
        index = torch.full((n,), POISON - 2 ** 32, dtype=torch.int32, device="cuda:0")
        count = torch.full((1,), -1, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        c = R.compact(rt.Paths(p, p.view(torch.int32)), mask, tens, out=(outs, index, count), stream=stream)
        assert c.n() == m, what
        assert c.count.data_ptr() == count.data_ptr() and c.index.data_ptr() == index.data_ptr()
        got = [_u32(o) for o in c.outs] + [_u32(c.index)]
        for g, h in zip(got[:4], host):
            assert np.array_equal(g[:m], h[sel]), what
            assert np.all(g[m:] == POISON), what   # nothing written at or beyond count
        assert np.array_equal(got[4][:m], want) and np.all(got[4][m:] == POISON), what
        if first is not None:
            assert all(np.array_equal(a, b) for a, b in zip(first, got)), what
        first = got


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 4097])
def test_compaction_equals_numpy(rt, R, n):
    rng = np.random.default_rng(n)
    for kind in SELECTIONS:
        for mask in (ALIVE, SHADOW, ALIVE | SHADOW):
            sel = _selection(kind, n, rng)
            paths, srcs = _records(n, sel, mask, rng)
            _check_compaction(rt, R, paths, srcs, mask, sel, (n, kind, mask))


@pytest.mark.parametrize("mask", [ALIVE, SHADOW, ALIVE | SHADOW])
def test_compaction_many_tiles(rt, R, mask):
    n = 300001
    assert n > 64 * TILE
    rng = np.random.default_rng(mask)
    sel = _selection("bernoulli", n, rng)
    paths, srcs = _records(n, sel, mask, rng)
    _check_compaction(rt, R, paths, srcs, mask, sel, (n, mask))


def test_compaction_index_only_and_no_index(rt, R):
    import torch
    n = 2500
    rng = np.random.default_rng(4)
    sel = _selection("bernoulli", n, rng)
    paths, srcs = _records(n, sel, SHADOW, rng)
    p = _dev(paths.view(F))
    torch.cuda.synchronize()
    c = R.compact(p, SHADOW)   # zero streams, index only
    m = c.n()
    assert m == sel.sum() and c.outs == [] and np.array_equal(_u32(c.index)[:m], np.nonzero(sel)[0])
    rays = _dev(srcs[1].view(F))
    out = torch.full((n, 8), -3.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    c = R.compact(p, SHADOW, (rays,), index=False, out=([out], None, None), stream=0)   # index = NULL
    assert c.index is None and c.n() == m
    got = _u32(out)
    assert np.array_equal(got[:m], srcs[1][sel]) and np.all(out[m:].cpu().numpy() == -3.0)
    e = torch.empty((0, 12), dtype=torch.float32, device="cuda:0")
    assert R.compact(e, ALIVE, stream=0).n() == 0   # n == 0: nothing launched, the count is the wrapper's


# ---- 6. connect / retire / average against numpy --------------------------------------------------------
def _finite(rng, shape):
    return (rng.standard_normal(shape) * 10.0 ** rng.integers(-3, 4, shape)).astype(F)


@pytest.mark.parametrize("n", [1, 65, 1000])
def test_connect_equals_numpy(rt, R, n):
    import torch
    rng = np.random.default_rng(n)
    paths = rng.integers(0, 2 ** 32, (n, 12), dtype=np.uint32)
    paths[:, 4:7] = _finite(rng, (n, 3)).view(np.uint32)
    contrib = _finite(rng, (n, 4))
    for use_index in (True, False):
        m = max(1, (2 * n) // 3)
        occ = rng.choice(np.array([0, 0, 1, 7], np.uint32), m)
        idx = rng.permutation(n)[:m].astype(np.uint32)
        if use_index and m > 1:
            idx[m // 2] = n + 5    # at or above n: skipped, never dereferenced
            occ[m // 2] = 0
        want = paths.copy()
        rows = idx if use_index else np.arange(m)
        hit = (occ == 0) & (rows < n)
        r = rows[hit]
        want[r, 4:7] = (paths[r, 4:7].view(F) + contrib[r, 0:3]).view(np.uint32)
        pad = torch.full((n + 2, 12), -9.25, dtype=torch.float32, device="cuda:0")
        pad.view(torch.int32)[1:n + 1] = _dev(paths)
        d_con, d_occ, d_idx = _dev(contrib), _dev(occ), _dev(idx)
        torch.cuda.synchronize()
        R.connect(pad[1:n + 1], d_con, d_occ, index=d_idx if use_index else None, m=m)
        R.wait()
        got = _u32(pad[1:n + 1])
        assert np.array_equal(got, want), (n, use_index)
        changed = np.nonzero((got != paths).any(axis=1))[0]
        assert set(changed) <= set(r.tolist()) and np.array_equal(got[:, [0, 1, 2, 3, 7, 8, 9, 10, 11]],
                                                                  paths[:, [0, 1, 2, 3, 7, 8, 9, 10, 11]])
        assert torch.all(pad[0] == -9.25).item() and torch.all(pad[-1] == -9.25).item()


@pytest.mark.parametrize("n", [1, 65, 1000])
def test_retire_equals_numpy(rt, R, n):
    import torch
    rng = np.random.default_rng(100 + n)
    tags = n + 3
    paths = rng.integers(0, 2 ** 32, (n, 12), dtype=np.uint32)
    paths[:, 7] = rng.integers(0, 4, n)
    paths[:, 11] = rng.permutation(tags)[:n]
    if n > 1:
        paths[n // 2, 7] = 0
        paths[n // 2, 11] = tags          # at or above `tags`: skipped
        paths[n // 2 - 1, 7] = 2
        paths[n // 2 - 1, 11] = 0xFFFFFFF0
    want = np.full((tags + 2, 4), POISON, np.uint32)
    dead = ((paths[:, 7] & ALIVE) == 0) & (paths[:, 11] < tags)
    want[1 + paths[dead, 11], 0:3] = paths[dead, 4:7]
    want[1 + paths[dead, 11], 3] = np.float32(1).view(np.uint32)
    pad = _dev(np.full((tags + 2, 4), POISON, np.uint32)).view(torch.float32)
    p = _dev(paths.view(F))
    torch.cuda.synchronize()
    R.retire(p, pad[1:tags + 1], stream=0)
    torch.cuda.synchronize()
    assert np.array_equal(_u32(pad), want), n   # only dead records' tags, guard rows intact
    assert np.array_equal(_u32(p), paths)


@pytest.mark.parametrize("n", [1, 65, 1000])
def test_average_equals_numpy(rt, R, n):
    import torch
    rng = np.random.default_rng(200 + n)
    for spp in (1, 2, 5):
        s = _finite(rng, (n, spp, 4))
        tot = s[:, 0, 0:3]
        for k in range(1, spp):
            tot = tot + s[:, k, 0:3]
        want = np.concatenate([tot / F(spp), np.ones((n, 1), F)], axis=1).astype(F)
        d = _dev(s.reshape(n * spp, 4))
        torch.cuda.synchronize()
        got = R.average(d, spp)
        R.wait()
        assert same(got.cpu().numpy(), want), (n, spp)
    with pytest.raises(rt.RTError):
        R.average(torch.zeros((65, 4), dtype=torch.float32, device="cuda:0"), 65)


# ---- 7. the loop against the frame ----------------------------------------------------------------------
LOOPS = [(name, "wavefront") for name in FRAMES] + [("c1", "megakernel")]


@pytest.mark.parametrize("name,pipeline", LOOPS)
def test_path_trace_equals_frame(rt, assets, name, pipeline):
    """Frame 0 from library calls only against the frame the same Renderer draws, all four
    channels and the ray totals; and that frame against one a Renderer draws without any query."""
    import torch
    what, W, H, spp, mb, mode = FRAMES[name]
    sc = textured_scene(rt, assets) if what == "textured" else rt.Scene.preset(what, assets)

    def renderer():
        r = make_renderer(rt, sc, W, H, pipeline, seed=SEED)
        r.samplesPerPixel, r.maxBounces, r.shadingMode = spp, mb, mode
        return r

    Rn = renderer()
    images, totals = [], []
    for batch in (True, False):
        img = Rn.path_trace(batch_samples=batch)
        torch.cuda.synchronize()
        images.append(img.cpu().numpy())
        totals.append(dict(Rn.last_path_trace))
    Rn.draw()
    Rn.wait()
    frame, st = Rn.radiance(), Rn.stats()
    print(f"{name} {pipeline}: {totals[0]}")
    for img, t in zip(images, totals):
        assert img.shape == (H, W, 4)
        assert same(img, frame) and img[..., :3].any()
        assert (t["closest_rays"], t["shadow_rays"], t["paths"]) == (st.closest_rays, st.shadow_rays, st.paths)
        assert 0 < t["rounds"] <= mb * (mb + 1) + 1
    Rn.close()
    R2 = renderer()
    R2.draw()
    R2.wait()
    assert same(R2.radiance(), frame)   # the queries did not disturb the frame
    R2.close()


# ---- 8. streams ---------------------------------------------------------------------------------------------
def test_path_trace_on_a_side_stream(rt, assets):
    import torch
    what, W, H, spp, mb, mode = FRAMES["c1"]
    Rn = make_renderer(rt, rt.Scene.preset(what, assets), W, H, "wavefront", seed=SEED)
    Rn.samplesPerPixel, Rn.maxBounces, Rn.shadingMode = spp, mb, mode
    want = Rn.path_trace().cpu().numpy()
    side = torch.cuda.Stream()
    a = torch.randn((2048, 2048), device="cuda:0")
    torch.cuda.synchronize()
    for _ in range(4):
        a = a @ a * 1e-3            # other work queued on the default stream
    img = Rn.path_trace(stream=side.cuda_stream)
    side.synchronize()
    assert same(img.cpu().numpy(), want)
    torch.cuda.synchronize()
    Rn.close()


def test_two_compactions_on_two_streams(rt, R):
    """Back to back on two streams with no host wait between them: each call's tile counts and
    selection words are its own query slot's."""
    import torch
    n = 200000
    rng = np.random.default_rng(8)
    jobs = []
    for mask in (ALIVE, SHADOW):
        sel = _selection("bernoulli", n, rng)
        paths, srcs = _records(n, sel, mask, rng)
        p, rays = _dev(paths.view(F)), _dev(srcs[1])
        jobs.append((mask, sel, paths, srcs, p, rays))
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    cs = [R.compact(p, mask, (rays, p), stream=s.cuda_stream) for (mask, _, _, _, p, rays), s in zip(jobs, (s1, s2))]
    for c, (mask, sel, paths, srcs, p, rays) in zip(cs, jobs):
        m = c.n()
        assert m == sel.sum()
        assert np.array_equal(_u32(c.outs[0])[:m], srcs[1][sel]) and np.array_equal(_u32(c.outs[1])[:m], paths[sel])
        assert np.array_equal(_u32(c.index)[:m], np.nonzero(sel)[0])
    # the per-slot storage is device memory the context accounts for: 132 B per tile, two slots at least
    assert R.stats().device_bytes >= 2 * 132 * ((n + TILE - 1) // TILE)
    torch.cuda.synchronize()


# ---- 9. errors on the device path ----------------------------------------------------------------------------
def test_compact_errors_leave_the_context_usable(rt, R):
    import torch
    A, L = rt._abi, rt.lib()
    E = A.RT_ERR_INVALID_ARG
    n = 500
    rng = np.random.default_rng(12)
    sel = _selection("bernoulli", n, rng)
    paths, srcs = _records(n, sel, ALIVE, rng)
    p, src = _dev(paths.view(F)), _dev(srcs[1])
    dst = torch.zeros_like(src)
    dst2 = torch.zeros_like(p)
    index = torch.zeros((n + 1,), dtype=torch.int32, device="cuda:0")
    count = torch.zeros((1,), dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    vp = C.c_void_p

    def call(pairs, mask=ALIVE, k=None, idx=index.data_ptr(), on=False):
        arr = (A.CompactStream * max(len(pairs), 1))()
        for j, (s, d, w) in enumerate(pairs):
            arr[j].src, arr[j].dst, arr[j].words = s, d, w
        args = (R._ctx, vp(p.data_ptr()), n, mask, arr, len(pairs) if k is None else k, vp(idx) if idx else None,
                vp(count.data_ptr()))
        return L.rt_compact_paths_on(*args, None) if on else L.rt_compact_paths(*args)

    good = (src.data_ptr(), dst.data_ptr(), 2)
    assert call([(src.data_ptr(), src.data_ptr(), 2)]) == E             # dst is its own src
    assert call([good, (p.data_ptr(), dst.data_ptr(), 3)]) == E         # two streams into one dst
    assert call([(src.data_ptr(), p.data_ptr(), 2)]) == E               # dst is paths
    assert call([(src.data_ptr(), dst.data_ptr(), 5)]) == E and call([(src.data_ptr(), dst.data_ptr(), 0)]) == E
    assert call([good], mask=0) == E
    assert call([good] * 4 + [good], k=5) == E
    assert call([good], idx=index.data_ptr() + 2) == E and call([good], idx=index.data_ptr() + 2, on=True) == E
    assert call([(src.data_ptr() + 8, dst.data_ptr(), 2)]) == E
    assert b"" != L.rt_last_error(R._ctx)
    R.wait()
    assert torch.all(dst == 0).item() and torch.all(dst2 == 0).item() and torch.all(index == 0).item()   # nothing was launched
    # the context is still usable: the next compaction is correct
    assert call([good, (p.data_ptr(), dst2.data_ptr(), 3)], idx=index.data_ptr() + 4) == A.RT_OK
    R.wait()
    m = int(count.cpu()[0])
    assert m == sel.sum()
    assert np.array_equal(_u32(dst)[:m], srcs[1][sel]) and np.array_equal(_u32(dst2)[:m], paths[sel])
    assert np.array_equal(_u32(index)[1:m + 1], np.nonzero(sel)[0])
    # the Python layer checks its tensors
    for bad in (dict(paths=p[:, :8]), dict(streams=(src[:10],)), dict(streams=(src.to(torch.float64),)),
                dict(streams=(src,) * 5), dict(out=([dst], None)), dict(streams=(src,), out=([dst[:5]], None, None)),
                dict(index=index), dict(paths=paths)):
        kw = dict(paths=p, mask=ALIVE, streams=())
        kw.update(bad)
        with pytest.raises(ValueError):
            R.compact(**kw)
    with pytest.raises(ValueError):
        R.connect(p, torch.zeros((n, 4), device="cuda:0"), index[:5], m=6)
    with pytest.raises(ValueError):
        R.retire(p, torch.zeros((n, 3), device="cuda:0"))
