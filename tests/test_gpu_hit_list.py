"""wf_shade shades hits only: each block compacts the hits of its batches of queue entries into a
dense list (an LDS ring of entry indices and hit records) and runs a shading pass per 256 of them,
so a missed ray takes no lane.  Every frame here is compared with the CPU oracle bit for bit --
radiance, depth, motion, closest / shadow / path counts -- on shapes chosen for the list's
boundaries: partial batches and a last pass with fewer than 256 hits (hit counts that are no
multiple of the wave or the block), empty lists, several bulk rounds before the finish launch, the
counting kernels, a tile split, the extra-sample pass (a second pass through the same rounds) and
the hit sort, which bypasses the list."""
import numpy as np
import pytest

from helpers import make_renderer

pytestmark = pytest.mark.gpu

# "wavefront-tail<N>": the default device-driven rounds with a finish threshold of N paths, so a
# small frame runs several bulk rounds and then the finish launch; the others: helpers._VARIANTS
# (wavefront-bulk: host-driven, every bounce through extend / shade / connect)
def _renderer(rt, scene, W, H, variant, seed, graphs=None, **kw):
    if variant.startswith("wavefront-tail"):
        R = rt.Renderer(scene, W, H, pipeline="wavefront", tail_paths=int(variant[len("wavefront-tail"):]), seed=seed, **kw)
    else:
        R = make_renderer(rt, scene, W, H, variant, seed=seed, **kw)
    if graphs is not None:
        R.set_graphs(graphs)
    return R


def _frame(R):
    R.wait()
    depth, motion, _ = R.aux()
    st = R.stats()
    return R.radiance(), depth, motion, (st.closest_rays, st.shadow_rays, st.paths)


def _assert_oracle(got, o, what=""):
    g, depth, motion, counts = got
    assert np.array_equal(g[..., :3], o["radiance"][..., :3]), what
    assert np.array_equal(depth, o["depth"]) and np.array_equal(motion, o["motion"]), what
    assert counts == (o["closest_rays"], o["shadow_rays"], o["paths"]), what


def _moved(rt, cam, dx):
    c = rt.Camera()
    c.position = type(cam.position)(cam.position.x + dx, cam.position.y, cam.position.z, 0.0)
    c.right, c.up, c.forward = cam.right, cam.up, cam.forward
    return c


# ---- the shared case: C1 (an open room: misses start at bounce 1), 96x64, 2 spp, 4 bounces, two
# frames; the oracle renders it once (from the first renderer's uniforms: every variant draws the same)
_W, _H, _SEED = 96, 64, 7


def _c1_frames(rt, assets, variant, graphs=None, counting=False, frames=2):
    scene = rt.Scene.preset("c1", assets)
    R = _renderer(rt, scene, _W, _H, variant, _SEED, graphs)
    R.samplesPerPixel, R.maxBounces = 2, 4
    if counting:
        R.set_counting(True)
    us, out = [], []
    for _ in range(frames):
        us.append(R.draw())
        out.append(_frame(R))
    rnd = R.random
    R.close()
    return scene, us, rnd, out


@pytest.fixture(scope="module")
def c1_ref(rt, orc, assets):
    """The oracle's two frames of the shared case (every variant draws the same uniforms)."""
    scene, us, rnd, _ = _c1_frames(rt, assets, "wavefront-bulk")
    osc = orc.OracleScene(scene.desc())
    prev = motion = None
    res = []
    for u in us:
        o = osc.render(u, rnd, accum_in=prev, motion_in=motion)
        prev, motion = o["radiance"], o["motion"]
        res.append(o)
    return res


@pytest.mark.parametrize("variant", ["wavefront-bulk", "wavefront-mixed", "wavefront-tail1024"])
def test_pipeline_variants(rt, assets, c1_ref, variant):
    """Frames captured as graphs and frames enqueued launch by launch give equal bits, the oracle's."""
    _, _, _, on = _c1_frames(rt, assets, variant, graphs=True)
    _, _, _, off = _c1_frames(rt, assets, variant, graphs=False)
    for f in range(2):
        _assert_oracle(on[f], c1_ref[f], (variant, "graphs", f))
        _assert_oracle(off[f], c1_ref[f], (variant, "eager", f))
        for a, b in zip(on[f], off[f]):
            assert np.array_equal(a, b)


def test_hit_sort(rt, assets, c1_ref):
    """The sorted shade path reads the sort's output, not the lists; extend still stores every record."""
    _, _, _, out = _c1_frames(rt, assets, "wavefront-bulk-sort")
    for f in range(2):
        _assert_oracle(out[f], c1_ref[f], f)


@pytest.mark.parametrize("variant", ["wavefront-bulk", "wavefront-tail1024"])
def test_counting_kernels(rt, assets, c1_ref, variant):
    """wf_trace<false, true>: the counting frame equals the plain one, its ray counts the oracle's."""
    _, _, _, plain = _c1_frames(rt, assets, variant, frames=1)
    _, _, _, cnt = _c1_frames(rt, assets, variant, counting=True, frames=1)
    for a, b in zip(plain[0], cnt[0]):
        assert np.array_equal(a, b)
    _assert_oracle(cnt[0], c1_ref[0], variant)


# ---- list boundaries ---------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["wavefront-bulk", "wavefront-tail2"])
@pytest.mark.parametrize("W,H,spp", [(8, 8, 1), (1, 1, 1), (40, 30, 3)])
def test_partial_flushes(rt, orc, assets, variant, W, H, spp):
    """64 paths (one wave of one block), one path, and 3600 paths: batches whose hit counts are no
    multiple of 64 or 256, and last passes with a partly filled list."""
    scene = rt.Scene.preset("c1", assets)
    R = _renderer(rt, scene, W, H, variant, 13)
    R.samplesPerPixel, R.maxBounces = spp, 4
    u = R.draw()
    got = _frame(R)
    rnd = R.random
    R.close()
    _assert_oracle(got, orc.OracleScene(scene.desc()).render(u, rnd), (variant, W, H))


def test_every_primary_ray_misses(rt, orc, assets):
    """The camera looks away from the room: round 0's lists stay empty, no shading pass runs and
    round 1 finds an empty queue.  Three frames back to back, two in flight."""
    W, H = 64, 48
    scene = rt.Scene.preset("c1", assets)
    R = _renderer(rt, scene, W, H, "wavefront-tail1024", 5, frames_in_flight=2)
    R.samplesPerPixel, R.maxBounces = 1, 3
    cam = R.camera
    P = type(cam.position)
    away = rt.Camera()
    away.position, away.up = cam.position, cam.up
    away.right = P(-cam.right.x, -cam.right.y, -cam.right.z, 0.0)
    away.forward = P(-cam.forward.x, -cam.forward.y, -cam.forward.z, 0.0)
    R.camera = away
    us = [R.draw() for _ in range(3)]
    got = _frame(R)
    rnd = R.random
    R.close()
    osc = orc.OracleScene(scene.desc())
    prev = motion = None
    for u in us:
        o = osc.render(u, rnd, accum_in=prev, motion_in=motion)
        prev, motion = o["radiance"], o["motion"]
    _assert_oracle(got, o)
    assert not np.any(got[0][..., :3])
    assert got[3] == (W * H, 0, W * H)   # closest rays = paths, no shadow ray


def test_tile_split(rt, orc, assets):
    """tiles=(16, r, 3) on 72x40 (ragged in both directions): each rank's tiles equal the full
    frame's (the oracle's), and the ranks' counts add up to it."""
    import torch
    W, H, T, n = 72, 40, 16, 3
    scene = rt.Scene.preset("c1", assets)

    def renderer():
        R = _renderer(rt, scene, W, H, "wavefront-bulk", 5)
        R.samplesPerPixel, R.maxBounces = 2, 3
        return R

    full = renderer()
    u = full.draw()
    ref = _frame(full)
    _assert_oracle(ref, orc.OracleScene(scene.desc()).render(u, full.random))
    full.close()
    canvas = np.zeros_like(ref[0])
    total = np.zeros(3, np.int64)
    tx = (W + T - 1) // T
    for rank in range(n):
        R = renderer()
        R.draw(tiles=(T, rank, n))
        cnt = R.tile_count(T, rank, n)
        buf = torch.empty((cnt, T, T, 4), dtype=torch.float32, device="cuda")
        R.pack_tiles(T, rank, n, buf.data_ptr())
        R.wait()
        torch.cuda.synchronize()
        packed = buf.cpu().numpy()
        st = R.stats()
        total += (st.closest_rays, st.shadow_rays, st.paths)
        R.close()
        for k in range(cnt):
            tid = rank + k * n
            x0, y0 = (tid % tx) * T, (tid // tx) * T
            w, h = min(T, W - x0), min(T, H - y0)
            canvas[y0:y0 + h, x0:x0 + w] = packed[k, :h, :w]
    assert np.array_equal(canvas, ref[0])
    assert tuple(total) == ref[3]


@pytest.mark.parametrize("variant", ["wavefront-bulk", "wavefront-tail64"])
def test_extra_sample_pass(rt, orc, assets, variant):
    """Motion-adaptive sampling under a camera move: frame 1's extra samples run as a second pass
    through the same bulk rounds (more of them than the finish threshold, so its rounds shade)."""
    W, H = 48, 32
    scene = rt.Scene.preset("c1", assets)
    R = _renderer(rt, scene, W, H, variant, 13)
    R.samplesPerPixel, R.maxBounces = 2, 3
    assert R.useMotionAdaptiveSampling
    cam0 = R.camera
    osc = orc.OracleScene(scene.desc())
    prev = motion = None
    for f in range(2):
        R.camera = _moved(rt, cam0, 0.4 * f)
        u = R.draw()
        got = _frame(R)
        o = osc.render(u, R.random, accum_in=prev, motion_in=motion)
        prev, motion = o["radiance"], o["motion"]
    R.close()
    assert o["paths"] > W * H * 2 + 64   # extra samples ran, more of them than the finish threshold
    _assert_oracle(got, o, variant)
