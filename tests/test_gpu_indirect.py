"""Device-count queries on the device (the count= forms of Renderer.trace / resolve / shade /
compact / connect / retire and path_trace(device_counts=True) -> the rt_*_indirect entry points;
launch_count in csrc/rt_kernels.h, the rq_* kernels in csrc/rt_query.hip).

An indirect query over arrays of `max` records with *count = c must give, in its first c records,
what the direct query gives with n = c, bit for bit, and leave every byte after them alone: the
rest of the `max` records and a 64-record guard tail behind them, both filled with a byte sentinel
before the call.  A count above max clamps to max.  A compaction's count feeds the next queries with
no host wait between them, and the whole loop run that way renders the frame rt_render_frame
renders.

No test here gives the device anything it does not handle by design: the count-0 and clamp cases
check a bound, they do not cross it, and bad arguments are rejected on the host before any launch."""
import ctypes as C

import numpy as np
import pytest

import surface_ref as sr
from helpers import make_renderer, textured_scene
from test_gpu_shade import FRAMES
from test_shade_host import SEED

pytestmark = pytest.mark.gpu
ALIVE, SHADOW = 1, 2
GUARD = 64                       # records behind `max` that no launch may touch
SENT = 0xA5A5A5A5                # the sentinel byte 0xA5 in every byte
MAXES = (65, 1030, 3 * 1024 + 5)  # one wave + 1; across a compaction tile; fewer effective tiles than sized ones
TOTAL = MAXES[-1] + GUARD
IMG_W, IMG_H = 64, 50            # the virtual image the 3141 camera records are cut from


def _cases():
    out = []
    for mx in MAXES:
        cs = [c for c in (0, 1, 63, 64, 65) if c < mx] + [mx] + ([2 * 1024 + 1] if mx == MAXES[-1] else [])
        out += [(mx, c, c) for c in cs]
        out.append((mx, mx + 1000, mx))   # clamp: behaves as n = max
    return out


CASES = _cases()
IDS = [f"max{mx}-count{c}" for mx, c, _ in CASES]


def bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def sentinel(rows, cols=None, dtype=None):
    import torch
    shape = (rows,) if cols is None else (rows, cols)
    return torch.full(shape, SENT - 2 ** 32, dtype=torch.int32, device="cuda:0").view(dtype or torch.int32)


def word(v):
    import torch
    return torch.tensor([v], dtype=torch.int32, device="cuda:0")


def untouched(t, start):
    return bool(np.all(bits(t[start:]) == SENT))


@pytest.fixture(scope="module")
def R(rt, assets):
    r = rt.Renderer(rt.Scene.preset("c1", assets), 7, 5, seed=5)
    yield r
    r.close()


@pytest.fixture(scope="module")
def D(rt, R):
    """TOTAL records of every kind, made once by the direct queries and never written again:
    camera rays of a 64 x 50 image, their hits, surfaces and materials, and the paths, next rays,
    shadow rays and contributions of one shading step (mixed ALIVE / SHADOW flags)."""
    import torch
    u = rt.uniforms_default(IMG_W, IMG_H)
    u.camera = rt.camera_default(IMG_W, IMG_H)
    u.samplesPerPixel = 1
    rnd = torch.from_numpy(rt.random_offsets(9, IMG_W, IMG_H).view(np.int32)).to("cuda:0")
    torch.cuda.synchronize()
    rays, paths0 = R.camera_paths(0, n=TOTAL, uniforms=u, random_offsets=rnd, stream=0)
    hits = R.trace(rays, stream=0)
    S = R.resolve(rays, hits, stream=0)
    paths = paths0.buffer.clone()
    sh = R.shade(rays, S, paths, max_bounces=4, stream=0)
    pi = paths.view(torch.int32)
    pi[::9, 7] = pi[::9, 7] & ~ALIVE          # every camera path of the room goes on: end every ninth
    torch.cuda.synchronize()
    flags = bits(paths)[:, 7]
    assert (flags & ALIVE).any() and not (flags & ALIVE).all() and (flags & SHADOW).any() and not (flags & SHADOW).all()
    rng = np.random.default_rng(3)
    occluded = torch.from_numpy(rng.choice(np.array([0, 0, 1, 7], np.int32), TOTAL)).to("cuda:0")
    return dict(rays=rays, paths0=paths0.buffer, hits=hits, S=S, paths=paths, next=sh.next_rays, shadow=sh.shadow_rays,
                contrib=sh.contrib, occluded=occluded)


# ---- 1. each of the seven queries: the first c records, and nothing else ------------------------------
@pytest.mark.parametrize("mx,c,eff", CASES, ids=IDS)
@pytest.mark.parametrize("any_hit", [False, True], ids=["closest", "any"])
def test_trace(R, D, mx, c, eff, any_hit):
    import torch
    cols = None if any_hit else 8
    out = sentinel(mx + GUARD, cols, None if any_hit else torch.float32)
    cnt = word(c)
    want = R.trace(D["rays"][:eff], any_hit=any_hit, stream=0)
    got = R.trace(D["rays"][:mx], any_hit=any_hit, out=out[:mx], stream=0, count=cnt)
    torch.cuda.synchronize()
    got = got if any_hit else got.buffer
    want = want if any_hit else want.buffer
    assert got.data_ptr() == out.data_ptr() and got.shape[0] == mx      # returned at full length
    assert np.array_equal(bits(out[:eff]), bits(want)) and untouched(out, eff)


@pytest.mark.parametrize("mx,c,eff", CASES, ids=IDS)
def test_resolve(R, D, mx, c, eff):
    import torch
    surf, mat = sentinel(mx + GUARD, 16, torch.float32), sentinel(mx + GUARD, 12, torch.float32)
    want = R.resolve(D["rays"][:eff], D["hits"].buffer[:eff], stream=0)
    R.resolve(D["rays"][:mx], D["hits"].buffer[:mx], out=(surf[:mx], mat[:mx]), stream=0, count=word(c))
    torch.cuda.synchronize()
    assert np.array_equal(bits(surf[:eff]), bits(want.buffer)) and untouched(surf, eff)
    assert np.array_equal(bits(mat[:eff]), bits(want.material_buffer)) and untouched(mat, eff)


@pytest.mark.parametrize("mx,c,eff", CASES, ids=IDS)
def test_shade(rt, R, D, mx, c, eff):
    import torch
    S = D["S"]
    cut = lambda k: rt.Surface(S.buffer[:k], S.buffer[:k].view(torch.int32), S.material_buffer[:k],
                               S.material_buffer[:k].view(torch.int32))
    p_want, p_got = D["paths0"][:eff].clone(), D["paths0"][:mx + GUARD].clone()
    outs = [sentinel(mx + GUARD, cols, torch.float32) for cols in (8, 8, 4)]
    want = R.shade(D["rays"][:eff], cut(eff), p_want, max_bounces=4, stream=0)
    R.shade(D["rays"][:mx], cut(mx), p_got[:mx], max_bounces=4, out=tuple(o[:mx] for o in outs), stream=0, count=word(c))
    torch.cuda.synchronize()
    assert np.array_equal(bits(p_got[:eff]), bits(p_want))
    assert np.array_equal(bits(p_got[eff:]), bits(D["paths0"][eff:mx + GUARD]))   # paths past the count: as they were
    for o, w in zip(outs, (want.next_rays, want.shadow_rays, want.contrib)):
        assert np.array_equal(bits(o[:eff]), bits(w)) and untouched(o, eff)


@pytest.mark.parametrize("mx,c,eff", CASES, ids=IDS)
@pytest.mark.parametrize("mask", [ALIVE, SHADOW])
def test_compact_equals_numpy(R, D, mx, c, eff, mask):
    """Output, index and *count against numpy's boolean index on the first c records; *count is
    written for c == 0 too."""
    import torch
    p = D["paths"]
    streams = (D["next"][:mx], p[:mx], D["contrib"][:mx])
    outs = [sentinel(mx + GUARD, s.shape[1], torch.float32) for s in streams]
    index, count = sentinel(mx + GUARD), sentinel(1)
    R.compact(p[:mx], mask, streams, index=True, out=([o[:mx] for o in outs], index[:mx], count), stream=0, count=word(c))
    torch.cuda.synchronize()
    sel = (bits(p[:eff])[:, 7] & mask) != 0
    m = int(sel.sum())
    assert int(bits(count)[0]) == m
    for o, s in zip(outs, streams):
        assert np.array_equal(bits(o[:m]), bits(s[:eff])[sel]) and untouched(o, m)
    assert np.array_equal(bits(index[:m]), np.nonzero(sel)[0]) and untouched(index, m)
    # and the direct call with n = c agrees
    d_out, d_count = sentinel(mx, 8, torch.float32), sentinel(1)
    R.compact(p[:eff], mask, (D["next"][:eff],), index=False, out=([d_out[:eff]], None, d_count), stream=0)
    torch.cuda.synchronize()
    if eff:
        assert int(bits(d_count)[0]) == m and np.array_equal(bits(d_out[:m]), bits(outs[0][:m]))


@pytest.mark.parametrize("mx,c,eff", CASES, ids=IDS)
@pytest.mark.parametrize("use_index", [True, False], ids=["index", "identity"])
def test_connect(R, D, mx, c, eff, use_index):
    """The device count is m, the number of shadow rays; n stays the host's.  The paths are
    compared whole: the records no counted shadow ray names are as they were."""
    import torch
    n = mx + GUARD                       # every index entry is below n: the guard records are paths too
    idx = None
    if use_index:                        # distinct entries, as compact() makes them
        idx = torch.from_numpy(np.random.default_rng(mx).permutation(n)[:mx].astype(np.int32)).to("cuda:0")
    p_want, p_got = D["paths"][:n].clone(), D["paths"][:n].clone()
    R.connect(p_want, D["contrib"][:n], D["occluded"][:mx], index=idx, m=eff, stream=0)
    R.connect(p_got, D["contrib"][:n], D["occluded"][:mx], index=idx, m=mx, stream=0, count=word(c))
    torch.cuda.synchronize()
    assert np.array_equal(bits(p_got), bits(p_want))
    rows = bits(idx)[:eff].astype(np.int64) if use_index else np.arange(eff)
    named = np.zeros(n, bool)
    named[rows] = True
    assert np.array_equal(bits(p_got)[~named], bits(D["paths"][:n])[~named])


@pytest.mark.parametrize("mx,c,eff", CASES, ids=IDS)
def test_retire(R, D, mx, c, eff):
    import torch
    tags = IMG_W * IMG_H
    s_want, s_got = sentinel(tags + GUARD, 4, torch.float32), sentinel(tags + GUARD, 4, torch.float32)
    R.retire(D["paths"][:eff], s_want[:tags], stream=0)
    R.retire(D["paths"][:mx], s_got[:tags], stream=0, count=word(c))
    torch.cuda.synchronize()
    assert np.array_equal(bits(s_got), bits(s_want)) and untouched(s_got, tags)
    dead = (bits(D["paths"][:eff])[:, 7] & ALIVE) == 0
    assert int((bits(s_got)[:tags, 3] != SENT).sum()) == int(dead.sum())   # one sample per dead path below the count


# ---- 2. chaining without the host ---------------------------------------------------------------------
@pytest.mark.parametrize("side", [False, True], ids=["context-stream", "side-stream"])
def test_compaction_feeds_trace_and_resolve(R, D, side):
    """compact -> trace(count=) -> resolve(count=) with nothing between the calls, against the
    direct sequence with the count read back."""
    import torch
    n = MAXES[-1]
    st = torch.cuda.Stream() if side else None
    h = st.cuda_stream if side else None
    rays, hits = sentinel(n + GUARD, 8, torch.float32), sentinel(n + GUARD, 8, torch.float32)
    surf, mat = sentinel(n + GUARD, 16, torch.float32), sentinel(n + GUARD, 12, torch.float32)
    torch.cuda.synchronize()            # the inputs and the fills are on torch's stream
    cp = R.compact(D["paths"][:n], ALIVE, (D["next"][:n],), index=False, out=([rays[:n]], None, None), stream=h)
    R.trace(rays[:n], out=hits[:n], stream=h, count=cp)
    R.resolve(rays[:n], hits[:n], out=(surf[:n], mat[:n]), stream=h, count=cp.count)
    m = cp.n()                          # the first wait
    torch.cuda.synchronize()
    assert 0 < m < n and m == int(((bits(D["paths"][:n])[:, 7] & ALIVE) != 0).sum())
    d = R.compact(D["paths"][:n], ALIVE, (D["next"][:n],), index=False, stream=0)
    k = d.n()
    d_hits = R.trace(d.outs[0][:k], stream=0)
    d_S = R.resolve(d.outs[0][:k], d_hits, stream=0)
    torch.cuda.synchronize()
    assert k == m
    for got, want in ((rays, d.outs[0][:k]), (hits, d_hits.buffer), (surf, d_S.buffer), (mat, d_S.material_buffer)):
        assert np.array_equal(bits(got[:m]), bits(want)) and untouched(got, m)


# ---- 3. errors ------------------------------------------------------------------------------------------
def test_count_errors_leave_the_context_usable(rt, R, D):
    import torch
    A = rt._abi
    n = 1030
    p = D["paths"][:n]
    dst = sentinel(n, 8, torch.float32)
    count = word(n)
    arr = (A.CompactStream * 1)()
    arr[0].src, arr[0].dst, arr[0].words = D["next"].data_ptr(), dst.data_ptr(), 2
    vp = C.c_void_p

    def call(count_ptr, mx=n, out=None, on=False):
        dc = A.DeviceCount()
        dc.count, dc.max = count_ptr, mx
        other = sentinel(1) if out is None else out
        R._enqueue("rt_compact_paths", 0 if on else None, vp(p.data_ptr()), C.byref(dc), ALIVE, arr, 1, None,
                   vp(other.data_ptr()), form="_indirect")
        return other

    torch.cuda.synchronize()
    for bad in (dict(count_ptr=count.data_ptr(), out=count),       # count_out is the count compacted by
                dict(count_ptr=None),                              # NULL with max > 0
                dict(count_ptr=count.data_ptr() + 2),              # misaligned
                dict(count_ptr=count.data_ptr() + 2, on=True)):
        with pytest.raises(rt.RTError) as e:
            call(**bad)
        assert e.value.code == A.RT_ERR_INVALID_ARG, bad
    with pytest.raises(rt.RTError):
        R.compact(p, ALIVE, (D["next"][:n],), index=False, out=([dst], None, count), count=count)
    assert rt.lib().rt_trace_closest_indirect(R._ctx, None, None, None) == A.RT_ERR_INVALID_ARG   # cnt == NULL
    R.wait()
    assert untouched(dst, 0) and int(bits(count)[0]) == n          # nothing was launched
    # max == 0: RT_OK, nothing launched, nothing written, and the count pointer may be NULL
    out = call(None, mx=0)
    R.wait()
    assert untouched(out, 0) and untouched(dst, 0)
    for bad in (torch.zeros((2,), dtype=torch.int32, device="cuda:0"), torch.zeros((1,), dtype=torch.float32, device="cuda:0"),
                torch.zeros((1,), dtype=torch.int32), 5):
        with pytest.raises(ValueError):
            R.trace(D["rays"][:n], count=bad)
    # the context is still usable: the next compaction is correct
    out = call(count.data_ptr())
    R.wait()
    sel = (bits(p)[:, 7] & ALIVE) != 0
    assert int(bits(out)[0]) == sel.sum() and np.array_equal(bits(dst[:int(sel.sum())]), bits(D["next"][:n])[sel])


# ---- 4. statistics -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mx,c", [(65, 0), (1030, 63), (1030, 1030), (3 * 1024 + 5, 2 * 1024 + 1)])
def test_query_stats_count_the_effective_rays(R, D, mx, c):
    import torch
    torch.cuda.synchronize()
    want_hits = 0
    if c:
        R.trace(D["rays"][:c])
        want_hits = R.query_stats().hits
    before = R.query_stats().queries_total
    out = sentinel(mx, 8, torch.float32)
    cnt = word(c)
    torch.cuda.synchronize()
    R.trace(D["rays"][:mx], out=out, count=cnt)
    q = R.query_stats()
    assert (q.rays, q.hits, q.any_hit) == (c, want_hits, 0)
    assert q.queries_total == before + 1                 # c == 0 is a query too
    assert q.grid_blocks == (mx + 255) // 256            # what max gave


# ---- 5. the loop with its counts on the device ------------------------------------------------------------
LOOPS = [(name, "wavefront") for name in FRAMES] + [("c1", "megakernel")]


@pytest.mark.parametrize("name,pipeline", LOOPS)
def test_path_trace_device_counts_equals_frame(rt, assets, name, pipeline):
    import torch
    what, W, H, spp, mb, mode = FRAMES[name]
    sc = textured_scene(rt, assets) if what == "textured" else rt.Scene.preset(what, assets)

    def renderer():
        r = make_renderer(rt, sc, W, H, pipeline, seed=SEED)
        r.samplesPerPixel, r.maxBounces, r.shadingMode = spp, mb, mode
        return r

    Rn = renderer()
    want = Rn.path_trace()
    torch.cuda.synchronize()
    want = bits(want)
    runs = []
    for batch in (True, False) if name == "c1" else (True,):
        for lookahead in (0, 1, 3):
            img = Rn.path_trace(batch_samples=batch, device_counts=True, lookahead=lookahead)
            torch.cuda.synchronize()
            runs.append((batch, lookahead, bits(img), dict(Rn.last_path_trace)))
    Rn.draw()
    Rn.wait()
    frame, st = Rn.radiance(), Rn.stats()
    for batch, lookahead, img, t in runs:
        what_run = (name, pipeline, batch, lookahead, t)
        print(what_run)
        assert img.shape == (H, W, 4), what_run
        assert np.array_equal(img, want) and np.array_equal(img, sr.bits(frame)), what_run
        assert (t["closest_rays"], t["shadow_rays"], t["paths"]) == (st.closest_rays, st.shadow_rays, st.paths), what_run
        assert 0 < t["rounds"] <= mb * (mb + 1) + 1, what_run
        assert t["host_waits"] <= t["rounds"] + 1, what_run
    with pytest.raises(ValueError):
        Rn.path_trace(stream=None, device_counts=True)   # the renderer's own stream is not torch's to name
    Rn.close()
    R2 = renderer()
    R2.draw()
    R2.wait()
    assert np.array_equal(sr.bits(R2.radiance()), sr.bits(frame))   # a renderer that never ran a query draws the same frame
    R2.close()
